// nf_kernels.h -- hand-written gfx950 (CDNA4, wave64) kernels of the NeutFEM hot path.
//
// Everything here is fp64 and HBM-bound: stencil differences, batched tridiagonal line
// solves and streaming vector updates.  Design rules:
//   * A^-1 along a grid line is a first-order linear recurrence in each sweep direction, so it
//     is evaluated as a parallel scan of affine maps z -> a z + b instead of a serial Thomas
//     sweep: lanes of one wavefront scan an x-line with cross-lane shuffles (k_schur_x), and
//     y/z-lines are cut into register-resident segments whose summaries are combined through
//     LDS (k_schur_s).  No intermediate of the line solve ever goes to HBM.
//   * consecutive lanes always touch consecutive cells of the unit-stride x axis (coalesced
//     512 B - 1 KiB per wave instruction).
//   * reductions are two-stage with a fixed summation order (bitwise reproducible runs); the
//     scalars of CG (alpha, beta, stop test) never leave the device inside a solve.
#pragma once
#include <hip/hip_runtime.h>
#include "nf_outer.h"

// in-kernel cycle stamps: diagnostic builds only (-DNF_STAMPS, scratch library; never in the shipped one)
#ifdef NF_STAMPS
#define NF_STAMP(buf, i) do { if (buf) (buf)[i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define NF_STAMP(buf, i) do { } while (0)
#endif

// waves per SIMD the single-reduction variants of the slab z passes are compiled for (A/B builds: profiles/tools/r04_d_call.sh)
#ifndef NF_SR_Z1_WAVES
#define NF_SR_Z1_WAVES 3
#endif
#ifndef NF_SR_Z2_WAVES
#define NF_SR_Z2_WAVES 4
#endif
// where the staged y / z pass (k_schur_s, SV_STAGE) issues the next tile's copy: 0 = behind the first barrier, 1 = behind this tile's y loads (A/B builds)
#ifndef NF_STAGE_PLACE
#define NF_STAGE_PLACE 1
#endif

namespace nf {

// device-resident state of one CG solve (SchurSolver::SolveSchurImplicit, src/solvers.cpp:577-636)
struct CgScalars {
    double rr, pAp, alpha, beta, rr_new, tol_sq, rhs_norm, tol;
    int done, its, maxit;
    int pend;      // fused CG only: the x += alpha p of the last FIN_RR has not been applied yet (k_schur_x / k_cg_flush do it)
    // Error slot.  Every reduction of the solve that crosses ranks carries one extra double next to its sum: a rank that hit a local
    // error adds a non-zero value there, and a non-finite sum counts as an error too.  The kernel that consumes the reduced value sets
    // `done` and `err` from it -- on every rank from the same bits, so all ranks leave the solve at the same iteration with an error
    // instead of one returning early and the others waiting in the next collective.  1 = non-finite sum, 2 = a rank raised its flag.
    int err;
    // lean CG (CgLean): |r|^2 and the iteration count after the iteration of parity q, so that a kernel whose blocks all read
    // the values of parity q^1 can have its block 0 store those of parity q without a race
    double rr2[2]; int its2[2];
};

// Low-latency readback of a few scalars: a one-thread kernel copies them into host memory that the device can write (mapped, coherent)
// and then stores a sequence number with system-scope release; the host polls the sequence number.  Replaces a 100-byte D2H copy
// through the copy engine + stream drain, which costs ~30 us of idle GPU per check (once per group solve and per outer iteration).
struct HostPub { CgScalars cg; double out[8]; unsigned long long seq; };
__global__ void k_publish(const CgScalars *__restrict__ cg, const double *__restrict__ out, int nout, HostPub *hp, unsigned long long seq)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (cg) hp->cg = *cg;
    for (int i = 0; i < nout && i < 8; ++i) hp->out[i] = out[i];
    __threadfence_system();
    __hip_atomic_store(&hp->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Sum over the 64 lanes of a wavefront, result in every lane.  Data-parallel-primitive moves (row_shr 1/2/4/8 inside each row of
// 16 lanes, then row_bcast 15 and 31 across rows) instead of ds_bpermute shuffles: six dependent steps of a few cycles each where
// the LDS crossbar costs ~100 cycles per step -- the reductions sit on the critical path of every latency-bound kernel here.
// Fixed order (deterministic); out-of-row sources read as zero (bound_ctrl).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, true);
    return v + __hiloint2double(hi, lo);          // lanes outside ROW_MASK receive 0 (old = 0, bound_ctrl): v + 0
}
__device__ __forceinline__ double wave_sum(double v)
{
    v = dpp_add<0x111, 0xF>(v);                   // row_shr:1
    v = dpp_add<0x112, 0xF>(v);                   // row_shr:2
    v = dpp_add<0x114, 0xF>(v);                   // row_shr:4
    v = dpp_add<0x118, 0xF>(v);                   // row_shr:8  -> lane 15 of every row holds the row's sum
    v = dpp_add<0x142, 0xA>(v);                   // row_bcast:15 into rows 1 and 3 -> lanes 31 / 63 hold rows 0+1 / 2+3
    v = dpp_add<0x143, 0xC>(v);                   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// ---- cross-lane moves and scans of affine maps z -> A z + B with data-parallel primitives -------------------------------------
// lanes without a valid source (row / wavefront edge, or outside ROW_MASK) receive `old`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_get(double v, double old)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_above(double v) { return dpp_get<0x130, 0xF>(v, v); }   // wave_shl:1 = value of lane + 1
__device__ __forceinline__ double lane_below(double v) { return dpp_get<0x138, 0xF>(v, v); }   // wave_shr:1 = value of lane - 1
// Inclusive scan over groups of LPL consecutive lanes (LPL = 1, 2, 4 ... 64): afterwards lane li holds f_li o ... o f_0 of its group.
// row_shr 1/2/4/8 inside the rows of 16 lanes, then row_bcast 15 / 31 hand the totals of the lower rows upwards; no LDS crossbar.
#define NF_SCAN_STEP(CTRL, D) if (LPL > D) { double Ap = dpp_get<CTRL, 0xF>(A, 1.0), Bp = dpp_get<CTRL, 0xF>(B, 0.0); \
                                             if (pos < D) { Ap = 1.0; Bp = 0.0; } B = A * Bp + B; A = A * Ap; }
__device__ __forceinline__ void scan_maps_up(double &A, double &B, int LPL, int lane)
{
    const int pos = lane & ((LPL < 16 ? LPL : 16) - 1);
    NF_SCAN_STEP(0x111, 1) NF_SCAN_STEP(0x112, 2) NF_SCAN_STEP(0x114, 4) NF_SCAN_STEP(0x118, 8)
    if (LPL > 16) { const double Ap = dpp_get<0x142, 0xA>(A, 1.0), Bp = dpp_get<0x142, 0xA>(B, 0.0); B = A * Bp + B; A = A * Ap; }
    if (LPL > 32) { const double Ap = dpp_get<0x143, 0xC>(A, 1.0), Bp = dpp_get<0x143, 0xC>(B, 0.0); B = A * Bp + B; A = A * Ap; }
}
// The mirror image: lane li holds f_li o f_{li+1} o ... o f_{LPL-1}.  row_shl inside the rows; the totals of the higher rows come down
// through at most two crossbar reads (there is no downward row broadcast).
#define NF_SCAN_STEP_DN(CTRL, D) if (LPL > D) { double Ap = dpp_get<CTRL, 0xF>(A, 1.0), Bp = dpp_get<CTRL, 0xF>(B, 0.0); \
                                                if (pos + D >= W) { Ap = 1.0; Bp = 0.0; } B = A * Bp + B; A = A * Ap; }
__device__ __forceinline__ void scan_maps_down(double &A, double &B, int LPL, int lane)
{
    const int W = LPL < 16 ? LPL : 16, pos = lane & (W - 1);
    NF_SCAN_STEP_DN(0x101, 1) NF_SCAN_STEP_DN(0x102, 2) NF_SCAN_STEP_DN(0x104, 4) NF_SCAN_STEP_DN(0x108, 8)
    if (LPL > 16) {                                              // even rows take the suffix total of the row above (its first lane)
        const int src = (lane & ~31) + 16;
        double Ap = __shfl(A, src, 64), Bp = __shfl(B, src, 64);
        if (lane & 16) { Ap = 1.0; Bp = 0.0; }
        B = A * Bp + B; A = A * Ap;
    }
    if (LPL > 32) {                                              // the lower half takes the total of the upper half (lane 32)
        double Ap = __shfl(A, 32, 64), Bp = __shfl(B, 32, 64);
        if (lane >= 32) { Ap = 1.0; Bp = 0.0; }
        B = A * Bp + B; A = A * Ap;
    }
}

// thread t of the first 256 sums p[t], p[t + 256], ... in that order; the loads go out eight at a time (one memory round trip per
// eight terms instead of one per term: with 82 k partials -- split dot product at 512^3 -- the serial version took ~130 us)
__device__ __forceinline__ double strided_sum256(const double *__restrict__ p, int cnt)
{
    double s = 0.0;
    int i = threadIdx.x;
    if (threadIdx.x >= 256) return 0.0;
    for (; i + 7 * 256 < cnt; i += 8 * 256) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[i + j * 256];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; i < cnt; i += 256) s += p[i];
    return s;
}
// Workgroup barrier.  RAW (the staged y / z pass, see stage_issue): with a copy into LDS outstanding __syncthreads() is compiled as
// s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier -- it would wait for the next tile's vector in the middle of this one.  The raw form waits for
// the wave's own LDS traffic only; whoever reads the staged buffer waits for the copy by hand first.
template <bool RAW> __device__ __forceinline__ void block_bar()
{
    if constexpr (RAW) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }
    else __syncthreads();
}
// fixed-order block sum; result valid in thread 0.  sred: >= blockDim/64 doubles of LDS.
template <bool RAW = false>
__device__ __forceinline__ double block_sum(double v, double *sred)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    block_bar<RAW>();
    if (lane == 0) sred[w] = v;
    block_bar<RAW>();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < nw; ++i) s += sred[i];
    return s;
}

// three sums at once (the single-reduction CG's accumulation pass: p.q, q.q, r.q): one pair of barriers instead of three.  Same order of
// additions per sum as block_sum.  sred: >= 3 * blockDim / 64 doubles of LDS; results valid in thread 0.
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double *sred)
{
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) { sred[w] = a; sred[nw + w] = b; sred[2 * nw + w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0, sc = 0.0;
        for (int i = 0; i < nw; ++i) { sa += sred[i]; sb += sred[nw + i]; sc += sred[2 * nw + i]; }
        a = sa; b = sb; c = sc;
    }
}

// ---------------------------------------------------------------------------------------------
// second reduction stage + CG scalar logic.  One block of 256 threads.
// partials: nq rows of `stride` doubles; each local slab owns a segment [off, off+cnt) of every row.
struct PartSegs { int n; int off[16]; int cnt[16]; };
enum FinOp { FIN_RHS = 0, FIN_PAP = 1, FIN_RR = 2, FIN_SUM = 3 };

__device__ __forceinline__ int reduce_err(double total, double flag)       // error slot of an all-reduced sum (CgScalars::err)
{
    return flag != 0.0 ? 2 : ((total - total) != 0.0 ? 1 : 0);            // x - x is 0 for every finite x, NaN for inf / NaN
}
// ah (scalar-backed forms, may be null): the alpha history -- alpha of iteration j at ah[j % 8], for the x passes and the flush that apply several
// deferred x_sol updates at once (CgFuse::nold, nf_xsol_ring.h).  Eight doubles of their own, not part of CgScalars: the scalars travel whole
// to the host and through the one-XCD kernels.
__device__ __forceinline__ void cg_logic(int op, const double *tot, int nq, CgScalars *cg, double *out, double tol, int maxit, double flag = 0.0, double *ah = nullptr)
{
    if (op == FIN_RHS) { cg->err = 0; }
    if (op != FIN_SUM) { const int e = reduce_err(tot[0], flag); if (e) { cg->err = e; cg->done = 1; if (op == FIN_RHS) { cg->rr = tot[0]; cg->its = 0; cg->pend = 0; } return; } }
    if (op == FIN_RHS) {                       // src/solvers.cpp:587-592
        cg->rr = tot[0];
        cg->rhs_norm = sqrt(tot[0]);
        cg->tol = tol;
        cg->tol_sq = tol * tol * cg->rhs_norm * cg->rhs_norm;
        cg->done = 0; cg->its = 0; cg->maxit = maxit; cg->pend = 0;
        cg->rr2[0] = tot[0]; cg->its2[0] = 0;
        if (maxit <= 0) cg->done = 1;
    } else if (op == FIN_PAP) {                // src/solvers.cpp:602-606
        cg->pAp = tot[0];
        cg->pend = 0;                          // the x pass of this iteration has applied the deferred update
        if (fabs(tot[0]) < 1e-30) cg->done = 1;
        else { cg->alpha = cg->rr / tot[0]; if (ah) ah[cg->its & 7] = cg->alpha; }
    } else if (op == FIN_RR) {                 // src/solvers.cpp:613-631
        cg->rr_new = tot[0];
        cg->its += 1;
        cg->pend = 1;
        if (tot[0] < cg->tol_sq) { cg->rr = tot[0]; cg->done = 1; }
        else {
            cg->beta = tot[0] / cg->rr;
            cg->rr = tot[0];
            if (cg->its >= cg->maxit) cg->done = 1;
        }
    } else {
        for (int q = 0; q < nq; ++q) out[q] = tot[q];
    }
}

// reduce_only = 1: write the process-local sums to red[] (an all-reduce over ranks follows, then k_cg_logic)
__global__ __launch_bounds__(256) void k_finalize(int op, const double *__restrict__ partials, PartSegs segs, long stride,
                                                  int nq, CgScalars *__restrict__ cg, double *__restrict__ out,
                                                  double tol, int maxit, int reduce_only, double *__restrict__ red, const double *__restrict__ errsrc = nullptr,
                                                  double *__restrict__ ah = nullptr)
{
    __shared__ double sred[4];
    if ((op == FIN_PAP || op == FIN_RR) && !reduce_only) { if (cg->done) return; }
    double tot[4] = { 0, 0, 0, 0 };
    for (int q = 0; q < nq; ++q) {
        double acc = 0.0;
        for (int sgi = 0; sgi < segs.n; ++sgi) {
            double s = strided_sum256(partials + q * stride + segs.off[sgi], segs.cnt[sgi]);
            s = block_sum(s, sred);
            acc += s;
        }
        tot[q] = acc;
    }
    if (threadIdx.x != 0) return;
    // reduce_only: the sums go into an all-reduce over ranks, followed by this rank's error flag (errsrc, raised by the host)
    if (reduce_only) { for (int q = 0; q < nq; ++q) red[q] = tot[q]; if (errsrc) red[nq] = *errsrc; return; }
    cg_logic(op, tot, nq, cg, out, tol, maxit, 0.0, ah);
}
__global__ void k_cg_logic(int op, const double *__restrict__ red, int nq, CgScalars *__restrict__ cg, double *__restrict__ out,
                           double tol, int maxit, int with_flag, double *__restrict__ ah = nullptr)
{
    if (op == FIN_PAP || op == FIN_RR) { if (cg->done) return; }
    double tot[4] = { 0, 0, 0, 0 };
    for (int q = 0; q < nq; ++q) tot[q] = red[q];
    cg_logic(op, tot, nq, cg, out, tol, maxit, with_flag ? red[nq] : 0.0, ah);   // red[nq]: the all-reduced error flags of the ranks
    if (with_flag == 2) out[nq] = red[nq];                       // FIN_SUM of the outer iteration: the host reads the flags next to the sums
}

// Lean CG (undivided mesh, fused): the two k_finalize launches of an iteration disappear.  The consumer of a reduction sums
// the producer's block partials itself -- every block redundantly, in k_finalize's order, so all blocks get the same bits --
// and its block 0 stores the scalars for the kernels (and the host) that follow:
//   k_cg_rupdate sums the p.q partials of the last direction pass  -> alpha            (FIN_PAP, src/solvers.cpp:602-606)
//   the next iteration's x pass sums the |r|^2 partials of k_cg_rupdate -> beta, stop tests  (FIN_RR, :613-631)
// No block reads a field that another block of the same kernel writes: |r|^2 and the iteration count are kept per parity of
// the iteration (CgScalars::rr2 / its2); `done` is sticky and every block derives the same stop decision on its own.
// k_cg_lean_rr applies the FIN_RR step alone (idempotent: same inputs, same parity slot) so that the host, which reads the
// scalars at the end of a batch, sees the outcome of the batch's last iteration.
__device__ __forceinline__ double strided_total(const double *p, int cnt, double *sred);
// count < 0: partials[0] already holds the total (slab teams: k_finalize with reduce_only + the all-reduce over ranks put it there)
// flag_at > 0 (count >= 0): partials[flag_at] is the error slot that travelled with the partials (multi-rank teams all-reduce the
// vector of block partials itself and let the consumers sum it: no k_finalize launch on the critical path)
struct CgLean { CgScalars *st; const double *partials; int count; int par; int first; int flag_at; };
__device__ __forceinline__ double lean_total(const CgLean &lean, double *sred)
{
    return lean.count < 0 ? lean.partials[0] : strided_total(lean.partials, lean.count, sred);
}
// count < 0: partials[1] is the error slot that travelled with the total (sum of the ranks' flags)
__device__ __forceinline__ int lean_err(const CgLean &lean, double total)
{
    return reduce_err(total, lean.count < 0 ? lean.partials[1] : (lean.flag_at > 0 ? lean.partials[lean.flag_at] : 0.0));
}
__device__ __forceinline__ double strided_total(const double *p, int cnt, double *sred)   // blocks of >= 256 threads; result in every thread
{
    // summed by the first 256 threads only, so that blocks of any size (and k_finalize) produce the same bits: the other
    // threads add exact zeros
    double s = strided_sum256(p, cnt);
    s = block_sum(s, sred);
    if (threadIdx.x == 0) sred[0] = s;
    __syncthreads();
    s = sred[0];
    __syncthreads();
    return s;
}
// FIN_RR for the iteration of parity lean.par; returns true when the solve stops here.  *beta_out is valid when it continues.
// The scalars of the previous iteration are loaded up front (LeanPre), so that a kernel can have them -- and its own tile loads -- in
// flight while the partial sums are reduced, instead of paying one memory round trip after the other.
struct LeanPre { double rr_old, tol_sq; int its_old, maxit; };
__device__ __forceinline__ LeanPre lean_preload(const CgLean &lean)
{
    const CgScalars *st = lean.st; const int qo = lean.par ^ 1;
    LeanPre p; p.rr_old = st->rr2[qo]; p.tol_sq = st->tol_sq; p.its_old = st->its2[qo]; p.maxit = st->maxit;
    return p;
}
__device__ __forceinline__ bool lean_rr_step(const CgLean &lean, const LeanPre &pre, bool writer, double *sred, double *beta_out)
{
    CgScalars *st = lean.st;
    const int q = lean.par;
    const double rr_new = lean_total(lean, sred);
    const int e = lean_err(lean, rr_new);
    if (e) {                                                     // every block (and every rank) takes this branch from the same bits
        if (writer) { st->rr_new = rr_new; st->rr = rr_new; st->err = e; st->done = 1; }
        *beta_out = 0.0;
        return true;
    }
    const double rr_old = pre.rr_old;
    const int its_new = pre.its_old + 1;
    const bool conv = rr_new < pre.tol_sq;
    const bool stop = conv || its_new >= pre.maxit;
    const double beta = rr_new / rr_old;
    if (writer) {
        st->rr2[q] = rr_new; st->its2[q] = its_new;
        st->rr_new = rr_new; st->rr = rr_new; st->its = its_new; st->pend = 1;
        if (!conv) st->beta = beta;
        if (stop) st->done = 1;
    }
    *beta_out = beta;
    return stop;
}
__device__ __forceinline__ bool lean_rr_step(const CgLean &lean, bool writer, double *sred, double *beta_out)
{
    return lean_rr_step(lean, lean_preload(lean), writer, sred, beta_out);
}
// what a direction pass does between issuing its loads and using them (nothing, by default)
struct NoMid { __device__ __forceinline__ bool operator()(double &, double &) const { return false; } };
// hp: publish the scalars to the host right away (end of a batch of iterations: the host is polling, see HostPub)
__global__ __launch_bounds__(256) void k_cg_lean_rr(CgLean lean, HostPub *hp, unsigned long long seq)
{
    __shared__ double sred[4];
    if (!lean.st->done) {
        double beta;
        (void)lean_rr_step(lean, threadIdx.x == 0, sred, &beta);
    }
    if (hp && threadIdx.x == 0) {                                // the same thread wrote the scalars above
        hp->cg = *lean.st;
        __threadfence_system();
        __hip_atomic_store(&hp->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---------------------------------------------------------------------------------------------
// Single-reduction CG on slab teams (RT0-P0): ONE cross-rank reduction per iteration instead of two.
// The reference recurrence (src/solvers.cpp:577-636) needs p.Sp before it can form r_new and |r_new|^2 before it can form the next p:
// two dependent reductions.  Here the reduction of iteration j carries
//     red[0] = p_j.q_j   red[1] = q_j.q_j   red[2] = r_j.q_j   red[3] = |r_j|^2 (MEASURED, of the r the iteration started with)   red[4] = error flags
// and its consumer -- the first pass of iteration j+1 (the endpoint pass of the z lines, which reads p anyway) -- derives
//     alpha_j = |r_j|^2 / p.q          |r_{j+1}|^2 = |r_j|^2 - 2 alpha r.q + alpha^2 q.q   (the algebraic identity for |r - alpha q|^2)
//     beta_j  = |r_{j+1}|^2 / |r_j|^2
// and applies r -= alpha q, x += alpha p, p = r + beta p in one sweep.  The PREDICTED |r_{j+1}|^2 only feeds beta; the next reduction
// measures |r_{j+1}|^2 again, so nothing accumulates, and the stop test |r|^2 < tol^2 |b|^2 is taken on MEASURED values (one apply
// late: the solve that the reference ends after iteration j is ended here by the consumer of reduction j, with the same x_j).
// r.q is measured, not replaced by p.q: on IAEA-3D (blank assemblies with Sigma = 1e15, cond(S) ~ 1e17, |r|^2 swinging by ten orders
// of magnitude between consecutive iterations) the variants that lean on conjugacy or on r_new . r = 0 -- Chronopoulos-Gear, or
// |r_new|^2 = alpha^2 q.q - |r|^2 -- never converge (tests/test_single_reduction_cg.py shows it on the CPU oracle); this one needs
// the reference's iteration counts to within a few per cent there and identical counts on the well-conditioned benchmarks.
struct Cg1 { const double *red; CgScalars *st; int index; };   // index = iteration about to start (0: nothing to consume yet)
__device__ __forceinline__ bool cg1_step(const Cg1 &c, bool writer, double *alpha_out, double *beta_out)
{
    CgScalars *st = c.st;
    const double pq = c.red[0], qq = c.red[1], rq = c.red[2], rr = c.red[3], flag = c.red[4];
    const int j = c.index - 1;                                   // the iteration these sums belong to
    *alpha_out = 0.0; *beta_out = 0.0;
    const int e = flag != 0.0 ? 2 : ((((pq - pq) + (qq - qq)) + ((rq - rq) + (rr - rr))) != 0.0 ? 1 : 0);
    if (e) { if (writer) { st->err = e; st->done = 1; st->rr = rr; st->its = j; st->pend = 0; } return true; }
    if (j >= 1 && rr < st->tol_sq) { if (writer) { st->rr = rr; st->rr_new = rr; st->its = j; st->pend = 0; st->done = 1; } return true; }   // :624-628, on the measured |r_j|^2
    if (fabs(pq) < 1e-30) { if (writer) { st->pAp = pq; st->rr = rr; st->its = j; st->pend = 0; st->done = 1; } return true; }              // :604
    const double alpha = rr / pq;
    double rn = fma(alpha, fma(alpha, qq, -2.0 * rq), rr);       // |r - alpha q|^2
    if (!(rn > 0.0)) rn = 0.0;                                    // cancelled below rounding: restart from the residual (beta = 0)
    const double beta = rn / rr;
    const bool stop = j + 1 >= st->maxit;                        // the reference's loop bound: x still owes alpha_j p_j (k_cg_flush, pend)
    if (writer) {
        st->pAp = pq; st->alpha = alpha; st->beta = beta; st->its = j + 1; st->rr_new = rn;
        st->rr = stop ? rn : rr; st->pend = stop ? 1 : 0;
        if (stop) st->done = 1;
    }
    *alpha_out = alpha; *beta_out = beta;
    return stop;
}
// The four rows of block partials of one iteration -> red[0..3] (+ this rank's error flag -> red[4]): one wavefront per row, every lane
// sums the entries l, l + 64, ... of each slab's segment with eight loads in flight, one cross-lane sum at the end.  No barrier, no
// serial tail: ~3 us where k_finalize (one row and one segment at a time behind block-wide barriers) took 58 us for 4 x 8 x 256 partials.
__global__ __launch_bounds__(256) void k_reduce_rows(const double *__restrict__ partials, PartSegs segs, PartSegs segs3, long stride, double *__restrict__ red,
                                                     const double *__restrict__ errsrc)
{
    const int row = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double *p = partials + (long)row * stride;
    double s = 0.0;
    for (int sg = 0; sg < segs.n; ++sg) {
        const double *q = p + segs.off[sg]; const int cnt = row == 3 ? segs3.cnt[sg] : segs.cnt[sg];   // row 3 (|r|^2) comes from the endpoint pass, whose grid may differ
        int i = lane;
        for (; i + 7 * 64 < cnt; i += 8 * 64) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = q[i + j * 64];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; i < cnt; i += 64) s += q[i];
    }
    s = wave_sum(s);
    if (lane == 0) red[row] = s;
    if (threadIdx.x == 0 && errsrc) red[4] = *errsrc;
}
// the consumer's step on its own (end of a batch of iterations: the host is about to read the scalars), idempotent
__global__ void k_cg1_logic(Cg1 c, HostPub *hp, unsigned long long seq)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!c.st->done && c.index > 0) { double a, b; (void)cg1_step(c, true, &a, &b); }
    if (hp) { hp->cg = *c.st; __threadfence_system(); __hip_atomic_store(&hp->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
}

// ---------------------------------------------------------------------------------------------
// BuildMatrices, per-DOF diagonals (src/NeutFEM.cpp:1163-1302): C, fission and scatter matrices are diagonal
// (Legendre orthogonality): value = xs * detJ * C-hat_pp, C-hat_pp = prod_axes 2/(2 i_t + 1).  Output is SoA [p][e].
// mode 0 (C): entries <= 1e-14 dropped.  mode 1 (fission / scatter): P0: kept iff |xs| > 1e-14 (value xs*V);
// P>=1: element skipped iff |xs| < 1e-14, entries <= 1e-14 dropped (:1204-1302).
struct ChatArgs { int nloc; double c[27]; };
__global__ void k_cell_coef(const double *__restrict__ xs, double *__restrict__ out, const double *__restrict__ hx,
                            const double *__restrict__ hy, const double *__restrict__ hz, int nx, int ny, long N,
                            int mode, int dim, ChatArgs ch, const unsigned char *__restrict__ voidm = nullptr)
{
    // voidm (nf_set_void; fission, chi and scatter matrices only): the cross section of a void cell counts as zero, whatever was uploaded
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < N; e += (long)gridDim.x * blockDim.x) {
        const int ix = (int)(e % nx); const long r = e / nx; const int iy = (int)(r % ny); const int iz = (int)(r / ny);
        const double s = voidm && voidm[e] ? 0.0 : xs[e];
        if (ch.nloc == 1 && mode != 2) {
            const double V = hx[ix] * hy[iy] * hz[iz];
            double v = s * V;
            if (mode == 0) { if (!(fabs(v) > 1e-14)) v = 0.0; }
            else { if (!(fabs(s) > 1e-14)) v = 0.0; }
            out[e] = v;
        } else {
            double detJ = hx[ix] / 2.0;
            if (dim >= 2) detJ *= hy[iy] / 2.0;
            if (dim == 3) detJ *= hz[iz] / 2.0;
            const bool skip = mode >= 1 && fabs(s) < 1e-14;      // mode 2: AssembleWeightedMassMatrix (:1495-1529), any order
            for (int p = 0; p < ch.nloc; ++p) {
                double v = skip ? 0.0 : s * detJ * ch.c[p];
                if (!(fabs(v) > 1e-14)) v = 0.0;
                out[(long)p * N + e] = v;
            }
        }
    }
}
// host layout [e*nloc + p] <-> device layout [p*N + e]
__global__ void k_transpose_dofs(const double *__restrict__ in, double *__restrict__ out, long N, int nloc, int to_soa)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < N * nloc; i += gridDim.x * 256L) {
        const long e = to_soa ? i % N : i / nloc; const int p = to_soa ? (int)(i / N) : (int)(i % nloc);
        if (to_soa) out[i] = in[e * nloc + p]; else out[i] = in[(long)p * N + e];
    }
}

struct Geom {
    int dim, nx, ny, nz, k;
    const double *hx, *hy, *hz;
    // Line operators are stored for UNIT transverse scaling: for transverse Legendre mode a the whole chain matrix
    // (Dirichlet term included, src/NeutFEM.cpp:1458-1489) is T_a times the unit one, T_a = prod 2/(2 a_t + 1), so
    // the LDL^T multipliers are common to all modes and u = T^-1 t does not depend on T_a at all.
    // aLL/aLR: 1-D face block after the k bubbles of the cell have been condensed (RT0: [[2/3,1/3],[1/3,2/3]],
    // RT1: [[1/4,-1/12],..], RT2: [[2/15,1/30],..]); T0 = 2^(dim-1) is the mode-0 scaling (B-hat = -+T0 for RT0).
    double aLL, aLR, T0;
    int dir_lo[3], dir_hi[3];    // Dirichlet flags per direction (src/NeutFEM.cpp:2338-2347 attribute map)
};

// geometric factor of direction d for cell (ix,iy,iz), src/FEM.cpp:795-813 (2D quirk kept)
__device__ __forceinline__ double geom_factor(const Geom &G, int d, int ix, int iy, int iz)
{
    const double hx = G.hx[ix], hy = G.hy[iy], hz = G.hz[iz];
    if (G.dim == 1) return hx / 2.0;
    if (G.dim == 2) return d == 0 ? hy / hx : hx / hy;
    if (d == 0) return 2.0 * hx / (hy * hz);
    if (d == 1) return 2.0 * hy / (hx * hz);
    return 2.0 * hz / (hx * hy);
}
// Dirichlet diagonal term I_f(a) * 2 * D / T_a (src/NeutFEM.cpp:1350, 1458-1489): 2D, 4D/area, 8D/area
__device__ __forceinline__ double dirichlet_term(const Geom &G, int d, int ix, int iy, int iz, double D)
{
    double area = d == 0 ? G.hy[iy] * G.hz[iz] : d == 1 ? G.hx[ix] * G.hz[iz] : G.hx[ix] * G.hy[iy];
    double I = G.dim == 1 ? 1.0 : G.dim == 2 ? 2.0 / area : 4.0 / area;
    return I * 2.0 * D;
}
__device__ __forceinline__ void cell_a(const Geom &G, int d, int ix, int iy, int iz, double D, double &a2, double &a1)
{
    const double a = (1.0 / D) * geom_factor(G, d, ix, iy, iz);
    a2 = G.aLL * a; a1 = G.aLR * a;
    if (G.k == 0) {                                             // src/NeutFEM.cpp:1064 drop threshold on the real entries
        if (!(fabs(G.T0 * a2) > 1e-14)) a2 = 0.0;
        if (!(fabs(G.T0 * a1) > 1e-14)) a1 = 0.0;
    }
}

// One (direction, transverse mode) pass of the Schur apply for RT_k-P_m.  The phi moments (i along the line,
// transverse index a) of a cell couple to the line unknowns of mode a only:
//   faces    t_f = xR_{f-1} - xL_f,   xR = x_0 - sum_l eR_l G_l x_{l+1},  xL = x_0 + sum_l eL_l G_l x_{l+1}
//   solve    T_unit u = t             (bubbles condensed per cell: scalars because M^bb is diagonal for k <= 2)
//   bubbles  v_l = G_l x_{l+1} iM_l / c_e - (eL_l u_c + eR_l u_{c+1}),  c_e = factor_dir / D
//   output   y_0 += T_a (u_{c+1} - u_c),   y_{l+1} += T_a G_l v_l
// NB = number of bubble moments that exist in P_m (min(k, m)); NB = 0 is RT0-P0 (or RT_k-P0).
struct ModeArgs {
    double Ta;
    double eL[2], eR[2], Gc[2], iM[2];
    const double *x[3];          // moment arrays of the input vector: x[0] (along-index 0), x[1], x[2]
    double *y[3];
    const double *Cd[3];         // C diagonal of the same moments (first pass only)
    const double *D;             // diffusion coefficient per cell (for 1/c_e); used when NB > 0
    int dir;
};

// All transverse modes of one direction in ONE launch (they touch disjoint moments): the kernels get the ModeArgs of mode 0
// plus, per mode, T_a and the offset of its moments relative to mode 0's; the mode is the last grid dimension.
struct ModeTab { int n; double Ta[9]; long doff[9][3]; };
__device__ __forceinline__ ModeArgs select_mode(ModeArgs ma, const ModeTab &mt, int m, int nbp1)
{
    if (mt.n > 1) {
        ma.Ta = mt.Ta[m];
        for (int i = 0; i < nbp1; ++i) { const long o = mt.doff[m][i]; ma.x[i] += o; ma.y[i] += o; ma.Cd[i] += o; }
    }
    return ma;
}

// AssembleA + ApplyDirichletToA + SparseLU (src/NeutFEM.cpp:1036-1076,1328-1456; src/solvers.cpp:163)
// for one direction: one thread per grid line assembles the tridiagonal T of that line on the fly
// and stores its LDL^T factor cell-aligned: L[e] couples the lower to the upper face of cell e,
// DR[e] = 1/d'(upper face of e), D0[line] = 1/d'(first face).
// Slab decomposition (z lines only): if_lo / if_hi mark an interface with the neighbouring slab.  The
// interface face is a separator (partition method); the factored chain then covers the interior faces
// only: cells [fs, n-fe_off) with the edge cell's a2 added to the first/last chain diagonal.  Per line it
// also emits what the reduced (separator) system needs: alo/ahi = coupling a1 of the edge cells and
// hlo/hhi = this slab's half of the separator diagonal, a2_edge - a1_edge^2 (T_II^-1)[end,end].
// gfl = a1_lo a1_hi (T_II^-1)[first,last] measures the separator-to-separator coupling through the slab.
struct SlabOut { double *alo, *ahi, *hlo, *hhi, *gfl; };
// Cut-out cells (nf_set_void): voidm = one byte per cell, non-zero = void; inv_gamma = 1 / gamma of J.n = gamma phi on every face a kept
// cell shares with a void one.  A void cell adds nothing to the chain (cell_a gives (0, 0)), a kept|void face adds I_f / gamma to its
// diagonal -- I_f = dirichlet_term / (2 D) in the unit transverse scaling, with the area of the kept cell's face -- and a diagonal no kept
// cell and no Dirichlet term touches becomes 1 (identity row: void|void faces, natural domain faces of void cells).  A Dirichlet domain face
// of a void cell keeps its 2 D I term; it is decoupled (L = 0 on both sides of a void cell).  MASK = false is the code without any of this.
struct VoidArgs { const unsigned char *voidm; double inv_gamma; };
// The same mask for the vector kernels of the CG (DOF order [p][e]: the cell of entry i is i % ncell).  The direction passes know no mask:
// on a vector that is zero in the void cells B^T x is what the masked B gives and the line solves decouple by the factors, so only the
// void cells' own entries of S x come out wrong -- and p.q never sees them while p is zero there.  It is enough that r stays zero in the
// void cells (then p = r + beta p and x do): the MASK = true instantiations of the residual updates write 0 there and keep it out of |r|^2.
struct VoidMask { const unsigned char *m; long ncell; };
__device__ __forceinline__ bool void_entry(const VoidMask &vm, long i, long n) { return vm.m[n == vm.ncell ? i : i % vm.ncell] != 0; }
// y = Cd x in the void cells: what a plain Schur apply (nf_schur_apply) owes the caller there (C keeps the void cells; 0 for an x that vanishes there)
__global__ void k_void_apply_fix(const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ Cd, long n, VoidMask vm)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L)
        if (void_entry(vm, i, n)) y[i] = Cd[i] * x[i];
}
template <bool MASK>
__global__ void k_factor_lines(Geom G, int d, const double *__restrict__ D, double *__restrict__ L,
                               double *__restrict__ DR, double *__restrict__ D0, long nlines, int if_lo, int if_hi,
                               SlabOut so, VoidArgs va)
{
    const long line = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (line >= nlines) return;
    int n, ix = 0, iy = 0, iz = 0; long base, sl;
    const long nxy = (long)G.nx * G.ny;
    if (d == 0) { n = G.nx; iy = (int)(line % G.ny); iz = (int)(line / G.ny); base = line * G.nx; sl = 1; }
    else if (d == 1) { n = G.ny; ix = (int)(line % G.nx); iz = (int)(line / G.nx); base = iz * nxy + ix; sl = G.nx; }
    else { n = G.nz; ix = (int)(line % G.nx); iy = (int)(line / G.nx); base = line; sl = nxy; }
    int *ci = d == 0 ? &ix : d == 1 ? &iy : &iz;
    const int fs = if_lo ? 1 : 0, ce = if_hi ? n - 1 : n;       // chain cells [fs, ce)
    double a2, a1, ea2, ea1;
    // MASK (undivided meshes only): is cell c of the line void; the Robin term of the face between a void cell and kept cell c
    auto isv = [&](int c) -> bool { if constexpr (MASK) return va.voidm[base + (long)c * sl] != 0; else return false; };
    auto robin = [&](int c) -> double { *ci = c; return 0.5 * dirichlet_term(G, d, ix, iy, iz, 1.0) * va.inv_gamma; };
    // first chain face: lower contribution = Dirichlet term or the edge cell below
    *ci = fs;
    double Dc = D[base + (long)fs * sl];
    bool vc = isv(fs);
    cell_a(G, d, ix, iy, iz, Dc, a2, a1);
    if (MASK && vc) a2 = a1 = 0.0;
    double dprev;
    double alo = 0.0, a2lo = 0.0;
    if (if_lo) { *ci = 0; cell_a(G, d, ix, iy, iz, D[base], ea2, ea1); alo = ea1; a2lo = ea2; dprev = ea2 + a2; }
    else { *ci = fs; dprev = a2 + (G.dir_lo[d] ? dirichlet_term(G, d, ix, iy, iz, Dc) : 0.0); }
    if (MASK && dprev == 0.0) dprev = 1.0;
    double ahi = 0.0, a2hi = 0.0;
    if (if_hi) { *ci = n - 1; cell_a(G, d, ix, iy, iz, D[base + (long)(n - 1) * sl], ea2, ea1); ahi = ea1; a2hi = ea2; }
    D0[line] = 1.0 / dprev;
    double prodl = 1.0, g00 = 1.0 / dprev;                      // (T^-1)[0,0] = sum_k (prod_{j<k} l_j)^2 / d'_k
    for (int c = fs; c < ce; ++c) {
        double diag_next, na2 = 0.0, na1 = 0.0;
        bool vn = false;
        if (c + 1 < ce) {
            *ci = c + 1;
            const double Dn = D[base + (long)(c + 1) * sl];
            cell_a(G, d, ix, iy, iz, Dn, na2, na1);
            if constexpr (MASK) { vn = isv(c + 1); if (vn) na2 = na1 = 0.0; }
            diag_next = a2 + na2;
            if constexpr (MASK) if (vc != vn) diag_next += robin(vc ? c + 1 : c);
        } else if (if_hi) {
            diag_next = a2 + a2hi;
        } else {
            *ci = c;
            diag_next = a2 + (G.dir_hi[d] ? dirichlet_term(G, d, ix, iy, iz, Dc) : 0.0);
        }
        if (MASK && diag_next == 0.0) diag_next = 1.0;
        const double l = a1 / dprev;
        const double dn = diag_next - l * a1;
        L[base + (long)c * sl] = l;
        DR[base + (long)c * sl] = 1.0 / dn;
        prodl *= -l; g00 += prodl * prodl / dn;
        dprev = dn;
        if (c + 1 < ce) { Dc = D[base + (long)(c + 1) * sl]; a2 = na2; a1 = na1; vc = vn; }
    }
    if (if_lo) { L[base] = 0.0; DR[base] = 0.0; }
    if (if_hi) { L[base + (long)(n - 1) * sl] = 0.0; DR[base + (long)(n - 1) * sl] = 0.0; }
    if (so.alo) {
        so.alo[line] = alo; so.ahi[line] = ahi;
        so.hlo[line] = a2lo - alo * alo * g00;
        so.hhi[line] = a2hi - ahi * ahi / dprev;                 // (T^-1)[last,last] = 1/d'_last
        so.gfl[line] = alo * ahi * prodl / dprev;
    }
}

// separator values of the partition method (slab interfaces).  The reduced system over the separators of a z line is
//   S_red(s) u_s - G_below u_{s-1} - G_above u_{s+1} = c_s,   c_s = c_hi(slab below) + c_lo(slab above),
// G_r = a_lo a_hi (T_II^-1)[first,last] of slab r (SlabOut::gfl) = coupling of a slab's two separators through it.  G decays
// like 0.27^planes: for thick slabs the system is diagonal to rounding (u = c / S_red, k_separators alone); for thin slabs
// a few Jacobi sweeps u <- (c + G_below u_{s-1} + G_above u_{s+1}) / S_red (k_sep_couple, one more neighbour exchange,
// k_sep_update) reach rounding level; the number of sweeps is fixed at build time from the measured coupling.
// Both sides of an interface evaluate the same expression in the same order, so their copies of u agree bitwise.
__global__ void k_separators(const double *__restrict__ clo, const double *__restrict__ chi, const double *__restrict__ rlo,
                             const double *__restrict__ rhi, const double *__restrict__ sinv_lo, const double *__restrict__ sinv_hi,
                             double *__restrict__ ulo, double *__restrict__ uhi, double *__restrict__ ctlo, double *__restrict__ cthi,
                             long nlines, long ntot, int if_lo, int if_hi, const CgScalars *__restrict__ cg)
{
    // entries: [transverse mode][line] (ntot = modes * nlines); S_red, G are per line (unit-scaled factors serve every mode)
    if (cg && cg->done) return;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= ntot) return;
    const long l = i % nlines;
    if (if_lo) { const double c = rlo[i] + clo[i]; ctlo[i] = c; ulo[i] = c * sinv_lo[l]; }   // below's c_hi + own c_lo (same order on both sides)
    if (if_hi) { const double c = chi[i] + rhi[i]; cthi[i] = c; uhi[i] = c * sinv_hi[l]; }   // own c_hi + above's c_lo
}
// what this slab contributes to its two separators through itself: to the upper one G u_lower, to the lower one G u_upper
__global__ void k_sep_couple(const double *__restrict__ gfl, const double *__restrict__ ulo, const double *__restrict__ uhi,
                             double *__restrict__ elo, double *__restrict__ ehi, long nlines, long ntot, int if_lo, int if_hi,
                             const CgScalars *__restrict__ cg)
{
    if (cg && cg->done) return;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= ntot) return;
    const bool both = if_lo && if_hi;
    const double g = gfl[i % nlines];
    if (if_hi) ehi[i] = both ? g * ulo[i] : 0.0;
    if (if_lo) elo[i] = both ? g * uhi[i] : 0.0;
}
// u = ((c + e_from_below) + e_from_above) / S_red ; relo = the slab below's e_hi, rehi = the slab above's e_lo
__global__ void k_sep_update(const double *__restrict__ ctlo, const double *__restrict__ cthi, const double *__restrict__ elo,
                             const double *__restrict__ ehi, const double *__restrict__ relo, const double *__restrict__ rehi,
                             const double *__restrict__ sinv_lo, const double *__restrict__ sinv_hi, double *__restrict__ ulo,
                             double *__restrict__ uhi, long nlines, long ntot, int if_lo, int if_hi, const CgScalars *__restrict__ cg)
{
    if (cg && cg->done) return;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= ntot) return;
    const long l = i % nlines;
    if (if_lo) ulo[i] = ((ctlo[i] + relo[i]) + elo[i]) * sinv_lo[l];
    if (if_hi) uhi[i] = ((cthi[i] + ehi[i]) + rehi[i]) * sinv_hi[l];
}
// S_red^-1 from the two halves (own + neighbour's)
__global__ void k_sred_inv(const double *__restrict__ own, const double *__restrict__ other, double *__restrict__ out, long n, int own_first)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < n) out[i] = 1.0 / (own_first ? own[i] + other[i] : other[i] + own[i]);
}

// BuildDiagonalSchurCache (src/NeutFEM.cpp:483-597): S_inv(e) = 1/(C_ee + sum_faces B_ef^2 / A_ff)
// Slabs: the A_ff of an interface z face sums the edge cells of both slabs; nb_lo / nb_hi hold the neighbour's a2 per
// z line (k_edge_a2, exchanged once per group at cache-build time), nullptr on a domain boundary.
__global__ void k_edge_a2(Geom G, const double *__restrict__ D, double *__restrict__ lo, double *__restrict__ hi, long nlines)
{
    const long line = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (line >= nlines) return;
    const int ix = (int)(line % G.nx), iy = (int)(line / G.nx);
    double a2, a1;
    cell_a(G, 2, ix, iy, 0, D[line], a2, a1); lo[line] = a2;
    cell_a(G, 2, ix, iy, G.nz - 1, D[(long)(G.nz - 1) * G.nx * G.ny + line], a2, a1); hi[line] = a2;
}
__global__ void k_diag_cache(Geom G, const double *__restrict__ D, const double *__restrict__ Cd,
                             double *__restrict__ Sinv, long N, const double *__restrict__ nb_lo, const double *__restrict__ nb_hi)
{
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int ix = (int)(e % G.nx); const long r = e / G.nx; const int iy = (int)(r % G.ny); const int iz = (int)(r / G.ny);
    const long nxy = (long)G.nx * G.ny;
    double S = Cd[e];
    const double b2 = G.T0;                                      // B^2 / A_ff = T0^2 / (T0 A_unit)
    for (int d = 0; d < G.dim; ++d) {
        const int c = d == 0 ? ix : d == 1 ? iy : iz;
        const int n = d == 0 ? G.nx : d == 1 ? G.ny : G.nz;
        const long sl = d == 0 ? 1 : d == 1 ? G.nx : nxy;
        double a2, a1, b2n, b1n;
        cell_a(G, d, ix, iy, iz, D[e], a2, a1);
        // lower face
        double Alo = a2, Ahi = a2;
        if (c > 0) {
            int jx = ix - (d == 0), jy = iy - (d == 1), jz = iz - (d == 2);
            cell_a(G, d, jx, jy, jz, D[e - sl], b2n, b1n); Alo += b2n;
        } else if (d == 2 && nb_lo) Alo += nb_lo[e % nxy];
        else if (G.dir_lo[d]) Alo += dirichlet_term(G, d, ix, iy, iz, D[e]);
        if (c + 1 < n) {
            int jx = ix + (d == 0), jy = iy + (d == 1), jz = iz + (d == 2);
            cell_a(G, d, jx, jy, jz, D[e + sl], b2n, b1n); Ahi += b2n;
        } else if (d == 2 && nb_hi) Ahi += nb_hi[e % nxy];
        else if (G.dir_hi[d]) Ahi += dirichlet_term(G, d, ix, iy, iz, D[e]);
        if (fabs(G.T0 * Alo) > 1e-14) S += b2 / Alo;
        if (fabs(G.T0 * Ahi) > 1e-14) S += b2 / Ahi;
    }
    Sinv[e] = fabs(S) > 1e-14 ? 1.0 / S : 0.0;
}

// ---------------------------------------------------------------------------------------------
// Schur apply, x direction (unit stride along the line).  One wavefront scans 64/LPL lines;
// a lane owns K consecutive cells per chunk of LPL*K cells, NCH chunks cover the line.
//   forward  z_{c+1} = t_{c+1} - L[c] z_c, w = z * dinv ; backward u_f = w_f - L[f] u_{f+1}   (ModeArgs: t, outputs)
// `first`: y_p = Cd_p x_p + ... (the x pass is the first to touch every moment), else accumulate.
typedef double nf_d2 __attribute__((ext_vector_type(2)));
template <bool NT = false>                                       // NT: streaming (non-temporal) loads, see ldg below
__device__ __forceinline__ void ld2(const double *p, long i, bool ok, bool vec, double &a, double &b, bool ok2)
{
    if (vec) {
        nf_d2 v = { 0.0, 0.0 };
        if (ok) v = NT ? __builtin_nontemporal_load(reinterpret_cast<const nf_d2 *>(p + i)) : *reinterpret_cast<const nf_d2 *>(p + i);
        a = v.x; b = v.y;
    } else if (NT) { a = ok ? __builtin_nontemporal_load(p + i) : 0.0; b = ok2 ? __builtin_nontemporal_load(p + i + 1) : 0.0; }
    else { a = ok ? p[i] : 0.0; b = ok2 ? p[i + 1] : 0.0; }
}
// Streaming loads for the big-mesh passes: every array of a pass is larger than the caches and read once per pass, and a load that
// carries the non-temporal hint does not push the lines the other streams still need out of L2 / MALL.  Tiled copy with the y / z
// access pattern of the 256^3 passes, no arithmetic (profiles/tools/r02/tile_copy.hip, one MI355X): 4.99 -> 5.92 TB/s (y), 4.87 -> 6.07 (z);
// non-temporal *stores* lose (5.00 / 4.88 alone, 5.40 / 5.54 combined).  Not for meshes that live in the caches between launches.
template <bool NT>
__device__ __forceinline__ double ldg(const double *p) { return NT ? __builtin_nontemporal_load(p) : *p; }
// wave-uniform array base + 32-bit byte offset: ONE VGPR addresses the same cell in every array of a pass (global_load v, v_off, s[base])
// instead of a 64-bit address per array and cell -- what keeps the many-array passes (chunked long lines; RT1 / RT2 y and z passes) out of
// scratch.  The host takes such a kernel only while one group's array stays below 4 GiB.
template <bool NT> __device__ __forceinline__ double ldo(const double *p, unsigned byte_off)
{
    const double *q = reinterpret_cast<const double *>(reinterpret_cast<const char *>(p) + byte_off);
    return NT ? __builtin_nontemporal_load(q) : *q;
}
__device__ __forceinline__ void sto(double *p, unsigned byte_off, double v) { *reinterpret_cast<double *>(reinterpret_cast<char *>(p) + byte_off) = v; }

// Fused CG (undivided mesh, any order: the x pass with all its transverse modes touches every moment exactly once): the
// vector updates that follow FIN_RR -- x_sol += alpha p and p = r + beta p
// (src/solvers.cpp:609,630) -- are deferred to the next iteration's x pass, which reads p anyway: p is read once instead
// of three times per iteration and one launch disappears.  Same operands, same expressions: bit-identical iterates.
// The last iteration's x_sol update is applied by k_cg_flush (CgScalars::pend).
// pout: where the new direction p = r + beta p goes (nullptr: in place).  The fused-direction launch (k_apply3) runs the x, y
// and z passes of one apply side by side, so the y / z blocks must still find the old p while the x blocks write the new
// one: they read p and r and form r + beta p themselves (mode "read-only fuse"), and the x blocks write into the other
// buffer of a pair.  Every site evaluates fma(beta, p, r) / fma(alpha, p, x_sol): same bits everywhere.
// Batched x_sol update (k_schur_x<..., XB>, RT0-P0; the slots and alpha entries come from nf_xsol_ring.h): x_sol is never read back by the
// iteration, so with a ring of M direction buffers (p = the slot read, pout = the slot written) the x pass leaves it alone in M-1 of M
// iterations (XB_SKIP: neither loaded nor stored) and every M-th pass (XB_APPLY) catches up: x_sol = fma(alpha_j, p_j, x_sol) for the
// nold = M-1 older directions old[0] .. old[nold-1], oldest first, with alpha_j = ah[(a0 + j) & 7] (cg_logic's alpha history: launches are queued ahead
// of the scalars), then today's fma(alpha, p, x_sol) with the direction the pass reads anyway.  The same chain per cell: the same bits.
enum { XB_NOW = 0, XB_SKIP = 1, XB_APPLY = 2 };
struct CgFuse { double *p; const double *r; double *xsol; double *pout; int nold; int a0; const double *ah; const double *old[7]; };

// Tables of distinct lines.  A core built from a few assembly types and axial zones on a uniform mesh has only a handful of DIFFERENT lines per
// direction (IAEA-3D at 256^3: 12 / 12 / 3 of 65 536), and lines with equal stored factors need those factors once: the streaming passes then
// read L, 1/d (and the C diagonal, x pass) from a table [id][cell] that stays in L2 instead of streaming 16 (24) bytes per cell from HBM.
// The ids are found on the stored factors themselves: a 128-bit fingerprint of every line's bit patterns (k_line_fp), grouped on the host,
// every line compared bit for bit with its group's representative (k_line_verify: a collision switches the direction's table off), the
// representatives' rows gathered (k_line_gather).  Same values, same arithmetic: the table path is bit-identical to the streaming path.
struct LineDict { const int *id = nullptr; int pitch = 0; };     // id per line of the group; doubles per table row (multiple of 16)
struct LineFp { unsigned long long lo, hi; };
__device__ __forceinline__ void line_span(int d, long line, int nx, int ny, int nz, long &base, long &sl, int &n)   // as in k_factor_lines
{
    const long nxy = (long)nx * ny;
    if (d == 0) { n = nx; base = line * nx; sl = 1; }
    else if (d == 1) { n = ny; base = (line / nx) * nxy + line % nx; sl = nx; }
    else { n = nz; base = line; sl = nxy; }
}
__device__ __forceinline__ void fp_mix(unsigned long long &a, unsigned long long &b, double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    a ^= u; a *= 0xff51afd7ed558ccdull; a ^= a >> 33;
    b = ((b << 27) | (b >> 37)) + u; b *= 0xc4ceb9fe1a85ec53ull; b ^= b >> 31;
}
// bits: how many low bits of the fingerprint are kept (128 = all; fewer only to provoke collisions in tests)
__global__ void k_line_fp(int d, int nx, int ny, int nz, const double *__restrict__ L, const double *__restrict__ DR, const double *__restrict__ D0,
                          const double *__restrict__ Cd, long nlines, int bits, LineFp *__restrict__ out)
{
    const long line = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (line >= nlines) return;
    long base, sl; int n;
    line_span(d, line, nx, ny, nz, base, sl, n);
    unsigned long long a = 0x9e3779b97f4a7c15ull, b = 0xd1b54a32d192ed03ull;
    fp_mix(a, b, D0[line]);
    for (int c = 0; c < n; ++c) {
        const long e = base + c * sl;
        fp_mix(a, b, L[e]); fp_mix(a, b, DR[e]);
        if (Cd) fp_mix(a, b, Cd[e]);
    }
    if (bits < 64) { b = 0; a &= bits <= 0 ? 0ull : (~0ull >> (64 - bits)); }
    else if (bits < 128) b &= bits == 64 ? 0ull : (~0ull >> (128 - bits));
    out[line].lo = a; out[line].hi = b;
}
// every line against the representative of its id, bit for bit; *mism counts the lines that differ
__global__ void k_line_verify(int d, int nx, int ny, int nz, const double *__restrict__ L, const double *__restrict__ DR, const double *__restrict__ D0,
                              const double *__restrict__ Cd, long nlines, const int *__restrict__ id, const int *__restrict__ rep, int *__restrict__ mism)
{
    const long line = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (line >= nlines) return;
    const long other = rep[id[line]];
    if (other == line) return;
    long base, sl, ob, osl; int n;
    line_span(d, line, nx, ny, nz, base, sl, n);
    line_span(d, other, nx, ny, nz, ob, osl, n);
    bool same = __double_as_longlong(D0[line]) == __double_as_longlong(D0[other]);
    for (int c = 0; c < n; ++c) {
        const long e = base + c * sl, o = ob + c * osl;
        same = same && __double_as_longlong(L[e]) == __double_as_longlong(L[o]) && __double_as_longlong(DR[e]) == __double_as_longlong(DR[o]);
        if (Cd) same = same && __double_as_longlong(Cd[e]) == __double_as_longlong(Cd[o]);
    }
    if (!same) atomicAdd(mism, 1);
}
// table rows [id][cell], pitch doubles apart (the tail of a row stays zero): tL, tR and, for x lines, tC
__global__ void k_line_gather(int d, int nx, int ny, int nz, const double *__restrict__ L, const double *__restrict__ DR, const double *__restrict__ Cd,
                              const int *__restrict__ rep, int nrows, int pitch, double *__restrict__ tL, double *__restrict__ tR, double *__restrict__ tC)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)nrows * pitch) return;
    const int row = (int)(i / pitch), c = (int)(i % pitch);
    long base, sl; int n;
    line_span(d, rep[row], nx, ny, nz, base, sl, n);
    const bool in = c < n; const long e = base + c * sl;
    tL[i] = in ? L[e] : 0.0; tR[i] = in ? DR[e] : 0.0;
    if (tC) tC[i] = in ? Cd[e] : 0.0;
}

// One wave-task of the x pass: 64/LPL lines, lane = (line of the task, position in the line).  Returns the lane's share of x.y.
// DPPS: cross-lane traffic of the scans through data-parallel primitives (VALU) instead of ds_bpermute (LDS crossbar).  That halves
// the latency of a lone wave-task (resident kernel: 14.2 k -> 10.9 k cycles per x pass) but costs VALU issue slots: with many waves
// per SIMD the crossbar version is faster (fused-direction launch at 128^3: 76.8 vs 82.9 us per CG iteration on the same box).
// DICT (streaming instantiations of RT0-P0 meshes whose lines repeat, see LineDict): L, DR and ma.Cd[0] point at the table of distinct lines
// and the line's row replaces its own cells -- plain loads (the table is meant to stay in L2), same shapes, bit-equal values.
template <int K, int NCH, bool VEC, int NB, class Mid = NoMid, bool DPPS = false, bool NT = false, bool DICT = false, int XB = XB_NOW>
__device__ __forceinline__ double schur_x_task(const ModeArgs &ma, const Geom &G, const double *__restrict__ L, const double *__restrict__ DR,
                                               const double *__restrict__ D0, int nx, int ny, long nlines, int lpl_log2, int first,
                                               long task, int lane, bool active, bool fuse, double f_alpha, double f_beta, const CgFuse &fz, Mid mid = Mid(),
                                               const LineDict &ld = LineDict())
{
    static_assert(K == 2, "two cells per lane and chunk");
    static_assert(!DICT || (NB == 0 && NT), "line tables: next to the streaming RT0-P0 instantiations only");
    static_assert(XB == XB_NOW || NB == 0, "batched x_sol update: RT0-P0 only");
    const int LPL = 1 << lpl_log2, LPW = 64 >> lpl_log2;
    const int li = lane & (LPL - 1), sub = lane >> lpl_log2;
    const long line = task * LPW + sub;
    const bool lv = active && line < nlines;
    const long base = lv ? line * nx : 0;
    const int iy = lv ? (int)(line % ny) : 0, iz = lv ? (int)(line / ny) : 0;
    long cbase = base;                                           // where the line's coefficients start: its own cells, or its row of the table
    if (DICT) cbase = lv ? (long)((unsigned)ld.id[line] * (unsigned)ld.pitch) : 0;
    constexpr bool NTC = NT && !DICT;
    double xm[NB + 1][NCH][K], yo[NB + 1][NCH][K], Ls[NCH][K], Rs[NCH][K], w[NCH][K], xL[NCH][K], xR[NCH][K], ic[NCH][K];
    double rq[NB + 1][NCH][K], sq[NB + 1][NCH][K], dq[NB > 0 ? NCH : 1][K];   // fused variants: r and x_sol of the same cells; D (1 / c_e)
    double *pw = fz.pout ? fz.pout : fz.p;
    // ---- loads only (every load of the pass is in flight before `mid` runs and before the first value is used)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c0 = (ch * LPL + li) * K;
        const bool ok = lv && c0 < nx, ok2 = lv && c0 + 1 < nx;
        ld2<NTC>(L, cbase + c0, ok, VEC, Ls[ch][0], Ls[ch][1], ok2);
        ld2<NTC>(DR, cbase + c0, ok, VEC, Rs[ch][0], Rs[ch][1], ok2);
#pragma unroll
        for (int q = 0; q <= NB; ++q) {
            ld2<NT>(ma.x[q], base + c0, ok, VEC, xm[q][ch][0], xm[q][ch][1], ok2);
            if (DICT && first) ld2<false>(ma.Cd[q], cbase + c0, ok, VEC, yo[q][ch][0], yo[q][ch][1], ok2);
            else ld2<NT>(first ? ma.Cd[q] : ma.y[q], base + c0, ok, VEC, yo[q][ch][0], yo[q][ch][1], ok2);
            if (fuse) {                                          // ma.x[q] points into p: the same offset addresses r and x_sol
                const long mo = (ma.x[q] - fz.p) + base + c0;
                ld2<NT>(fz.r, mo, ok, VEC, rq[q][ch][0], rq[q][ch][1], ok2);
                if (XB != XB_SKIP) ld2<NT>(fz.xsol, mo, ok, VEC, sq[q][ch][0], sq[q][ch][1], ok2);
            }
        }
        if (NB > 0) ld2<NT>(ma.D, base + c0, ok, VEC, dq[NB > 0 ? ch : 0][0], dq[NB > 0 ? ch : 0][1], ok2);
    }
    if (mid(f_alpha, f_beta)) return 0.0;
    double av[7];                                                // XB_APPLY: alpha of the older directions, oldest first (wave-uniform)
    if (XB == XB_APPLY) {
#pragma unroll
        for (int i = 0; i < 7; ++i) av[i] = i < fz.nold ? fz.ah[(fz.a0 + i) & 7] : 0.0;
    }
    // ---- the deferred CG update of these cells, then the face values
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c0 = (ch * LPL + li) * K;
        const bool ok = lv && c0 < nx, ok2 = lv && c0 + 1 < nx;
        if (fuse) {
#pragma unroll
            for (int q = 0; q <= NB; ++q) {
                const long mo = (ma.x[q] - fz.p) + base + c0;
                if (XB == XB_APPLY) {
                    // the older directions of these cells: loaded here, chunk by chunk, and not with the pass's other loads -- 14 doubles
                    // in flight per lane whatever NCH is, where 7 x NCH x K more registers would cost occupancy (NCH = 2) or spill (NCH = 8)
                    double o0[7], o1[7];
#pragma unroll
                    for (int i = 0; i < 7; ++i) if (i < fz.nold) ld2<NT>(fz.old[i], mo, ok, VEC, o0[i], o1[i], ok2);
#pragma unroll
                    for (int i = 0; i < 7; ++i) if (i < fz.nold) { sq[q][ch][0] = fma(av[i], o0[i], sq[q][ch][0]); sq[q][ch][1] = fma(av[i], o1[i], sq[q][ch][1]); }
                }
                double s0 = 0.0, s1 = 0.0;
                if (XB != XB_SKIP) { s0 = fma(f_alpha, xm[q][ch][0], sq[q][ch][0]); s1 = fma(f_alpha, xm[q][ch][1], sq[q][ch][1]); }
                xm[q][ch][0] = fma(f_beta, xm[q][ch][0], rq[q][ch][0]); xm[q][ch][1] = fma(f_beta, xm[q][ch][1], rq[q][ch][1]);
                if (VEC) {
                    if (ok) { if (XB != XB_SKIP) *reinterpret_cast<double2 *>(fz.xsol + mo) = make_double2(s0, s1);
                              *reinterpret_cast<double2 *>(pw + mo) = make_double2(xm[q][ch][0], xm[q][ch][1]); }
                } else {
                    if (ok) { if (XB != XB_SKIP) fz.xsol[mo] = s0; pw[mo] = xm[q][ch][0]; }
                    if (ok2) { if (XB != XB_SKIP) fz.xsol[mo + 1] = s1; pw[mo + 1] = xm[q][ch][1]; }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double pl = 0.0, pr = 0.0;
            ic[ch][j] = 0.0;
            if (NB > 0) {
                const double dd = dq[NB > 0 ? ch : 0][j];
                const bool okj = j == 0 ? ok : ok2;
                ic[ch][j] = okj ? dd / geom_factor(G, 0, c0 + j, iy, iz) : 0.0;      // 1 / c_e
#pragma unroll
                for (int l = 0; l < NB; ++l) { const double gx = ma.Gc[l] * xm[l + 1][ch][j]; pl += ma.eL[l] * gx; pr += ma.eR[l] * gx; }
            }
            xL[ch][j] = xm[0][ch][j] + pl; xR[ch][j] = xm[0][ch][j] - pr;
        }
    }
    const double d0 = lv ? D0[line] : 0.0;
    const double z0 = __shfl(-xL[0][0], 0, LPL);
    // ---- forward sweep over chunks
    double carry = z0;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        double xn = DPPS ? lane_above(xL[ch][0]) : __shfl_down(xL[ch][0], 1, LPL);
        double xc = 0.0;
        if (ch + 1 < NCH) xc = __shfl(xL[ch + 1 < NCH ? ch + 1 : ch][0], 0, LPL);
        if (li == LPL - 1) xn = xc;
        double t[K];
#pragma unroll
        for (int j = 0; j < K; ++j) t[j] = xR[ch][j] - (j + 1 < K ? xL[ch][j + 1 < K ? j + 1 : j] : xn);
        double A = 1.0, B = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) { B = t[j] - Ls[ch][j] * B; A = -Ls[ch][j] * A; }
        if (DPPS) scan_maps_up(A, B, LPL, lane);
        else for (int d = 1; d < LPL; d <<= 1) {
            const double Ap = __shfl_up(A, d, LPL), Bp = __shfl_up(B, d, LPL);
            if (li >= d) { B = A * Bp + B; A = A * Ap; }
        }
        const double Ae = DPPS ? lane_below(A) : __shfl_up(A, 1, LPL), Be = DPPS ? lane_below(B) : __shfl_up(B, 1, LPL);
        double z = li == 0 ? carry : Ae * carry + Be;
#pragma unroll
        for (int j = 0; j < K; ++j) { z = t[j] - Ls[ch][j] * z; w[ch][j] = z * Rs[ch][j]; }
        if (ch + 1 < NCH) carry = __shfl(z, LPL - 1, LPL);
    }
    // ---- backward sweep over chunks
    double ucarry = 0.0, dot = 0.0;
#pragma unroll
    for (int ch = NCH - 1; ch >= 0; --ch) {
        double Ln = DPPS ? lane_above(Ls[ch][0]) : __shfl_down(Ls[ch][0], 1, LPL);
        double Lc = 0.0;
        if (ch + 1 < NCH) Lc = __shfl(Ls[ch + 1 < NCH ? ch + 1 : ch][0], 0, LPL);
        if (li == LPL - 1) Ln = Lc;
        double Lup[K];
#pragma unroll
        for (int j = 0; j < K; ++j) Lup[j] = j + 1 < K ? Ls[ch][j + 1 < K ? j + 1 : j] : Ln;
        double A = 1.0, B = 0.0;
#pragma unroll
        for (int j = K - 1; j >= 0; --j) { B = w[ch][j] - Lup[j] * B; A = -Lup[j] * A; }
        if (DPPS) scan_maps_down(A, B, LPL, lane);
        else for (int d = 1; d < LPL; d <<= 1) {
            const double Ap = __shfl_down(A, d, LPL), Bp = __shfl_down(B, d, LPL);
            if (li + d < LPL) { B = A * Bp + B; A = A * Ap; }
        }
        const double Ae = DPPS ? lane_above(A) : __shfl_down(A, 1, LPL), Be = DPPS ? lane_above(B) : __shfl_down(B, 1, LPL);
        double u = li == LPL - 1 ? ucarry : Ae * ucarry + Be;
        double uv[K];
#pragma unroll
        for (int j = K - 1; j >= 0; --j) { u = w[ch][j] - Lup[j] * u; uv[j] = u; }
        if (ch > 0) ucarry = __shfl(uv[0], 0, LPL);
        double ulo = DPPS ? lane_below(uv[K - 1]) : __shfl_up(uv[K - 1], 1, LPL);
        double wprev = 0.0;
        if (ch > 0) wprev = __shfl(w[ch > 0 ? ch - 1 : 0][K - 1], LPL - 1, LPL);
        if (li == 0) ulo = (ch == 0 ? z0 * d0 : wprev) - Ls[ch][0] * uv[0];
        double yv[NB + 1][K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double lo = j == 0 ? ulo : uv[j > 0 ? j - 1 : 0];
            yv[0][j] = (first ? yo[0][ch][j] * xm[0][ch][j] : yo[0][ch][j]) + ma.Ta * (uv[j] - lo);
            dot += xm[0][ch][j] * yv[0][j];           // padded cells have x = 0
#pragma unroll
            for (int l = 0; l < NB; ++l) {
                const double v = ma.Gc[l] * xm[l + 1][ch][j] * ma.iM[l] * ic[ch][j] - (ma.eL[l] * lo + ma.eR[l] * uv[j]);
                yv[l + 1][j] = (first ? yo[l + 1][ch][j] * xm[l + 1][ch][j] : yo[l + 1][ch][j]) + ma.Ta * ma.Gc[l] * v;
                dot += xm[l + 1][ch][j] * yv[l + 1][j];
            }
        }
        const int c0 = (ch * LPL + li) * K;
#pragma unroll
        for (int q = 0; q <= NB; ++q) {
            if (VEC) { if (lv && c0 < nx) *reinterpret_cast<double2 *>(ma.y[q] + base + c0) = make_double2(yv[q][0], yv[q][K - 1]); }
            else {
#pragma unroll
                for (int j = 0; j < K; ++j) if (lv && c0 + j < nx) ma.y[q][base + c0 + j] = yv[q][j];
            }
        }
    }
    return dot;
}

template <int K, int NCH, bool VEC, int NB, bool NT = false, bool DICT = false, int XB = XB_NOW>
__global__ __launch_bounds__(256) void k_schur_x(ModeArgs ma0, ModeTab mt, Geom G, const double *__restrict__ L, const double *__restrict__ DR,
                                                 const double *__restrict__ D0, int nx, int ny, long nlines, int lpl_log2,
                                                 int first, int last, double *__restrict__ partials,
                                                 const CgScalars *__restrict__ cg, CgFuse fz, CgLean lean, LineDict ld = LineDict())
{
    __shared__ double sred[4];
    if (cg && cg->done) return;
    const ModeArgs ma = select_mode(ma0, mt, blockIdx.y, NB + 1);
    const bool lean_on = lean.st && !lean.first;                 // lean CG: this pass consumes the |r|^2 partials (FIN_RR)
    const bool fuse = fz.p != nullptr && (lean.st ? lean_on : cg->its > 0);
    const double alpha0 = fuse ? cg->alpha : 0.0, beta0 = (fuse && !lean.st) ? cg->beta : 0.0;
    LeanPre pre = { 0.0, 0.0, 0, 0 };
    if (lean_on) pre = lean_preload(lean);
    bool stopped = false;
    auto mid = [&](double &fa, double &fb) -> bool {             // runs with the pass's loads in flight
        (void)fa;
        if (lean_on) stopped = lean_rr_step(lean, pre, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0, sred, &fb);
        return stopped;
    };
    // bit 1 of `first`: XCD-contiguous block order (consecutive workgroups go round-robin to the 8 XCDs; each then walks one eighth of the lines)
    unsigned bx = blockIdx.x;
    if ((first & 2) && gridDim.x % 8 == 0) bx = (blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
    const double dot = schur_x_task<K, NCH, VEC, NB, decltype(mid), false, NT, DICT, XB>(ma, G, L, DR, D0, nx, ny, nlines, lpl_log2, first & 1, (long)bx * 4 + (threadIdx.x >> 6),
                                                                           threadIdx.x & 63, true, fuse, alpha0, beta0, fz, mid, ld);
    if (stopped) return;                                         // decided inside, the same in every block: nothing to reduce
    if (last && partials) {
        const double s = block_sum(dot, sred);
        if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + bx] = s;   // by position: the sum order does not depend on the block order
    }
}

// ---------------------------------------------------------------------------------------------
// Schur apply, y or z direction.  Thread = (ix lane, segment of SEG cells along the line) with
// the segment held in registers; segment summaries (affine maps) are exchanged through LDS.
// Always accumulates into y (the x pass ran first).  Grid: (ceil(nx/TX), n_outer).
// DIR (1 = y, 2 = z) only tags the instantiation so profilers list the two passes separately.
// SLAB = true (z lines of a slab with interfaces, RT0-P0): the kernel works on the interior chain of the
// slab-local line.  mode 1 = endpoint response (partition method, step 1): solve with the plain
// neighbour cells as boundary data, emit c_lo = -x_edge - a_lo u_first, c_hi = x_edge - a_hi u_last,
// touch no y.  mode 2 = final solve with the separator values u_lo/u_hi folded into the boundary data,
// accumulate y on the chain cells and on the edge cells.  mode 3 = the same solve, but instead of y it stores the face
// unknowns themselves, negated: the z currents of the slab (current reconstruction on decomposed meshes).
struct SlabArgs {
    int if_lo, if_hi, mode, xcd;
    // fold = 1 (mode 2, no separator sweeps): the separator values are formed here from the exchanged planes instead of by
    // k_separators -- u_lo = (r_lo + c_lo) S_red^-1, u_hi = (c_hi + r_hi) S_red^-1, the same expressions in the same order on
    // both sides of an interface, so the two copies agree bitwise
    int fold; const double *rlo, *rhi, *sinv_lo, *sinv_hi;
    int wsmin;                                // segments from which the wavefront scan of the summaries replaces the serial loops (0: default 64)
    // x || y on small slabs (team_schur_apply): the y pass runs beside the x pass on a second stream and stores its increment alone
    // (noacc) into a vector of its own; the accumulation pass of the z lines adds that vector (yadd) to y on the way
    int noacc; const double *yadd;
    const double *alo, *ahi, *ulo, *uhi;      // per line
    double *clo, *chi;                        // per line (mode 1 outputs)
    double *jz;                               // mode 3: J = -u on the slab's own z faces [((face) * nx * ny + line) * nfa + amode] (Sol_J_, src/solvers.cpp:228)
    double *jzb;                              // mode 3, RT1+: the z bubbles of the slab's cells [cell * ni + l + k * amode] (src/FEM.cpp:377-397)
    int nfa, ni, amode[9];                    // RT face / interior DOFs per face / cell and direction; RT transverse index of every P mode
    // single-reduction CG (template flag SR, see Cg1): mode 1 consumes the reduction of the previous iteration and carries r -= alpha q next
    // to the fused x / p update, leaving its blocks' shares of |r|^2 in sr_part; mode 2 leaves p.q, q.q and r.q in three rows of partials
    Cg1 sr; double *sr_r; const double *sr_q; double *sr_part; long sr_stride;
};
// One tile (TX columns x one line each, NSEG segments) of a y / z pass.  tid = thread index within the tile; threads with
// act == false only keep the barriers company.  acc: accumulate into y (the x pass ran before) or store the increment alone
// (fused-direction launch: every direction has an output vector of its own).  fro ("read-only fuse"): the input vector is
// r + beta x, formed on the fly (see CgFuse).  Returns the thread's share of x.y.
// V: the variant, a mask of SV_* bits.
// SV_FUSE (slab passes): the instantiation that can carry the fused CG update (r and x_sol of the cells in registers: 160 instead of
// 128 VGPRs); the accumulation / emit passes use the one without
// SV_NT (big meshes): streaming loads (ldg) of everything but the overlap cell
// SV_ZW (plain RT0-P0 lines): the pass's share of x.y is not summed as x_i y_i over the cells -- x.(S_d x) = T_a t^T A^-1 t with
// A = L D L^T is T_a sum_faces z_f^2 / d_f = T_a sum z_f w_f, and both factors are at hand in the forward sweep.  The x pass then
// contributes x.(C x + S_x x) and the consumer adds the three sets of partials: the backward half of a y / z pass needs no x at all
// (eight doubles fewer live through the scans, and the chunked long-line pass has nothing to re-read for its parked chunk).
// SV_SR (RT0-P0 slab passes): single-reduction CG, see SlabArgs::sr
// SV_DICT (plain RT0-P0 lines in the streaming regime, see LineDict): L and DR point at the table of distinct lines; a lane carries the byte
// offset of its line's row and reaches the cells of its segment from there -- contiguous along the line, plain loads, bit-equal values
// XC (k_cg_xcd: the producers of x and r are other workgroups of the SAME launch on the same XCD): every load of x and r bypasses the
// compute unit's L1 -- the overlap cell too
// SV_STAGE (table-backed plain lines, full-width tiles): a block walks tiles b, b + blocks, ... and the NEXT tile's x is copied into LDS while
// this one is scanned (stage_issue); xv comes out of that buffer, everything behind it is the unstaged pass: same values, same arithmetic
// FULL (a template flag beside V, SV_STAGE only; the host's s_full): the tile grid has no partial tile -- nx a multiple of TX, n = SEG NSEG, TX NSEG
// threads, no wavefront scan.  Every per-access predicate (act, valid, c < n) is then true at compile time except the one of the overlap cell
// behind a line's last segment, and y is addressed like the many-array passes (ldo / sto: wave-uniform base + 32-bit byte offset).  Same values,
// same arithmetic, same slot in `partials`
enum : unsigned { SV_FUSE = 1, SV_NT = 2, SV_ZW = 4, SV_SR = 8, SV_DICT = 16, SV_STAGE = 32, SV_ALL = 63 };   // bit order = the order of the report's "variant"
// The instantiations of k_schur_s: the shapes (16- and 32-cell segments for RT0-P0 only, slabs cut z lines only) and the bits that a shape admits.
// The kernel asserts this and the host instantiates exactly the combinations for which it holds.
constexpr bool schur_s_legal(int SEG, int DIR, bool SLAB, int NB, unsigned V)
{
    const bool p0 = NB == 0, s8 = p0 && SEG == 8;                // RT0-P0; its 8-cell segments
    const unsigned admits = (SLAB && p0 ? SV_FUSE : 0) | (s8 ? SV_NT : 0) | (!SLAB && p0 ? SV_ZW : 0) | (SLAB && s8 && DIR == 2 ? SV_SR : 0) | (!SLAB && (V & SV_NT) ? SV_DICT : 0)
                            | (!SLAB && s8 && (V & SV_NT) && (V & SV_DICT) ? SV_STAGE : 0);
    return (SEG == 4 || SEG == 8 || (p0 && (SEG == 16 || SEG == 32))) && (DIR == 2 || (DIR == 1 && !SLAB)) && NB >= 0 && NB <= 2 && !(V & ~admits);
}
// The staged pass's copy of one tile of x into LDS.  The image is the tile as it lies in memory: [cell][TX] doubles, src = the first cell of the
// tile's first column, rows sl doubles apart.  One wave-instruction writes 1 KiB lane-linear (no register destination), i.e. 1024 / (8 TX) whole
// rows: the lane's SOURCE address picks the row and lanes whose row lies past the line are switched off.  Needs TX a power of two in 8 .. 64,
// full-width tiles and 16-byte aligned rows (the host's s_stage).  The copy counts on vmcnt: the issuing wave waits for it by hand, and a barrier
// separates that wait from the first read of the buffer: every wave waits ahead of its stores (schur_s_tile), the block meets at the top of
// the next tile (k_schur_s).  The lane's row of the table of distinct lines travels the same way: the id of the next tile's line is asked for
// next to the copy, so that the table loads of a tile do not start with a dependent round trip.
struct StageCtx {
    const double *buf = nullptr, *next = nullptr;                // the staged image of THIS tile; where the next tile of this block starts (null: none)
    const int *next_id = nullptr;                                // LineDict::id of the next tile's first column
    int id = 0;                                                  // this lane's table row in THIS tile; replaced by the next tile's on the way
};
// REDO (the whole-tile form, which has no register to spare): the lane's part of the source address is formed again at every call instead of
// living across the tile loop
template <bool NT, bool REDO = false>
__device__ __forceinline__ void stage_issue(const double *buf, const double *src, int n, long sl, int TX)
{
    typedef __attribute__((address_space(1))) const void *gptr_t;
    typedef __attribute__((address_space(3))) void *lptr_t;
    int lane = threadIdx.x & 63; const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    if (REDO) asm volatile("" : "+v"(lane));
    const int lpr = TX >> 1, rpp = 64 / lpr;                     // lanes per row (16 bytes each), rows per 1-KiB piece
    const int rl = lane / lpr, cl = lane % lpr;
    const char *dst = reinterpret_cast<const char *>(buf);
    for (int p = w, np = (n + rpp - 1) / rpp; p < np; p += nw) {
        const int r = p * rpp + rl;
        if (r < n) __builtin_amdgcn_global_load_lds((gptr_t)(src + (long)r * sl + 2 * cl), (lptr_t)(dst + p * 1024), 16, 0, NT ? 2 : 0);   // aux 2: nt, as ldg<NT>
    }
}
template <int SEG, int DIR, bool SLAB, int NB, unsigned V = 0, class Mid = NoMid, bool XC = false, bool FULL = false>
__device__ __forceinline__ double schur_s_tile(const ModeArgs &ma, const Geom &G, const double *__restrict__ L, const double *__restrict__ DR,
                                               const double *__restrict__ D0, int n, long sl, long outer_stride, int nx, int TX, int NSEG,
                                               unsigned bx, unsigned by, unsigned bz, unsigned gy, int tid, bool act, double *sm,
                                               const SlabArgs &sa, const CgFuse &fz, bool fuse, bool fro, double f_alpha, double f_beta, bool acc,
                                               long long *stamp = nullptr, Mid mid = Mid(), double *extra = nullptr, const LineDict &ld = LineDict(),
                                               StageCtx *sg = nullptr)
{
    constexpr bool FUSE = V & SV_FUSE, NT = V & SV_NT, ZW = V & SV_ZW, SR = V & SV_SR, DICT = V & SV_DICT, STAGE = V & SV_STAGE;
    static_assert(SLAB || !(FUSE || SR), "fused update, single-reduction sums: slab passes (k_schur_s checks the rest: schur_s_legal)");
    static_assert(!FULL || (STAGE && !SLAB && NB == 0), "whole-tile form: the staged pass");
    const double *x = ma.x[0];                                   // no __restrict__: the fused slab pass rewrites this vector (fz.p)
    double *__restrict__ y = ma.y[0];
    const int T = TX * NSEG;
    // Segment summaries: every thread composes the maps before (after) its own serially from LDS.  From 64 segments on (lines of
    // >= 505 cells) whole wavefronts scan the summaries of a column with cross-lane shuffles instead (lane = segment, log2 steps)
    // and hand every thread its incoming value through LDS: one more barrier per sweep, which only pays for the longest loops
    // (measured on one box, s_wsmin: 512-cell lines 77 -> 72 us, but 256-cell lines 134 -> 141 us, 384-cell 513 -> 540 us, 128-cell
    // 59 -> 66 us).  Needs full, aligned wavefronts.
    // (one wavefront spans a column's summaries: at most 64 segments -- a wider scan would need shuffles across wavefronts; longer
    // lines keep the serial loops)
    const bool wscan = !FULL && NSEG >= (sa.wsmin > 0 ? sa.wsmin : 64) && NSEG <= 64 && (T & 63) == 0;
    const int NSP = wscan ? (NSEG | 1) : NSEG;                   // odd row length: conflict-free column-major rows
    const int TP = wscan ? TX * NSP : T;
    double *sA = sm, *sB = sm + TP, *sA2 = sm + 2 * TP, *sB2 = sm + 3 * TP, *sZ0 = sm + 4 * TP;
    // FULL (the host's s_full): every thread owns a segment of a column inside the mesh, and every cell of it lies on the line -- the predicates
    // below are true at compile time, and what is left is the overlap cell of a line's last segment
    act = FULL || (act && tid < T);
    const int ixl = act ? tid % TX : 0, seg = act ? tid / TX : 0;
    const int si = wscan ? ixl * NSP + seg : seg * TX + ixl;     // this thread's slot in the summary arrays
    const int ix = bx * TX + ixl;
    const bool valid = FULL || (act && ix < nx);
    long base = (long)by * outer_stride + ix;
    const long lineid = (long)by * nx + ix;
    const long lm = SLAB ? (long)bz * ((long)nx * gy) + lineid : 0;   // slab exchange planes: [mode][line]
    const long roff = fro ? (long)(fz.r - fz.p) : 0;                 // r relative to the input vector (same offset for every moment)
    // slab chain: cells [fs, fs+n) of the local line; x just outside the chain is real data (edge cells)
    double x_before = 0.0, x_after = 0.0, a_lo = 0.0, a_hi = 0.0, u_lo = 0.0, u_hi = 0.0, xe_lo = 0.0, xe_hi = 0.0;
    long edge_lo = 0, edge_hi = 0;
    if (SLAB) {
        const int fs = sa.if_lo ? 1 : 0;
        const int nloc = n;                                      // local cells on the line
        n = nloc - fs - (sa.if_hi ? 1 : 0);
        edge_lo = base; edge_hi = base + (long)(nloc - 1) * sl;
        base += (long)fs * sl;
        if (valid) {
            // the edge cells sit between a separator and the chain: towards the chain they contribute xR (lower edge) / xL (upper
            // edge), towards the separator xL / xR -- for RT0 all four are the cell value itself
            if (sa.if_lo) {
                a_lo = sa.alo[lineid]; x_before = x[edge_lo];
                if (fuse) { if (seg == 0) fz.xsol[edge_lo] = fma(f_alpha, x_before, fz.xsol[edge_lo]);
                            x_before = fma(f_beta, x_before, (SR && FUSE) ? fma(-f_alpha, sa.sr_q[edge_lo], fz.r[edge_lo]) : fz.r[edge_lo]); }
                xe_lo = x_before;
                if (NB > 0) {
                    const double g1 = ma.Gc[0] * ma.x[1][edge_lo], g2 = NB > 1 ? ma.Gc[1] * ma.x[2][edge_lo] : 0.0;
                    xe_lo = x_before + ma.eL[0] * g1 + (NB > 1 ? ma.eL[1] * g2 : 0.0);            // xL: towards the separator below
                    x_before = x_before - ma.eR[0] * g1 - (NB > 1 ? ma.eR[1] * g2 : 0.0);          // xR: towards the chain
                }
                if (sa.mode >= 2) { u_lo = sa.fold ? (sa.rlo[lm] + sa.clo[lm]) * sa.sinv_lo[lineid] : sa.ulo[lm]; x_before -= a_lo * u_lo; }
            }
            if (sa.if_hi) {
                a_hi = sa.ahi[lineid]; x_after = x[edge_hi];
                if (fuse) { if (seg == 0) fz.xsol[edge_hi] = fma(f_alpha, x_after, fz.xsol[edge_hi]);
                            x_after = fma(f_beta, x_after, (SR && FUSE) ? fma(-f_alpha, sa.sr_q[edge_hi], fz.r[edge_hi]) : fz.r[edge_hi]); }
                xe_hi = x_after;
                if (NB > 0) {
                    const double g1 = ma.Gc[0] * ma.x[1][edge_hi], g2 = NB > 1 ? ma.Gc[1] * ma.x[2][edge_hi] : 0.0;
                    xe_hi = x_after - ma.eR[0] * g1 - (NB > 1 ? ma.eR[1] * g2 : 0.0);             // xR: towards the separator above
                    x_after = x_after + ma.eL[0] * g1 + (NB > 1 ? ma.eL[1] * g2 : 0.0);           // xL: towards the chain
                }
                if (sa.mode >= 2) { u_hi = sa.fold ? (sa.chi[lm] + sa.rhi[lm]) * sa.sinv_hi[lineid] : sa.uhi[lm]; x_after += a_hi * u_hi; }
            }
        }
    }
    const bool wr = !SLAB || sa.mode == 2;
    const int c0 = seg * SEG;
    double xv[SEG + 1], Lv[SEG + 1], Rv[SEG], yo[SEG];          // xv: x_0 moment; for NB > 0 xL / xR are derived below
    double x1[NB > 0 ? SEG : 1], x2[NB > 1 ? SEG : 1], icv[NB > 0 ? SEG : 1];
    double xLn = 0.0;                                            // xL of the first cell of the next segment
    // ---- loads only.  Every load of this phase is issued before the first use of a loaded value: a use inside a predicated region
    // makes the compiler wait for ALL outstanding memory operations there (s_waitcnt vmcnt(0) per region), i.e. one memory round
    // trip per cell instead of one per phase (measured with in-kernel stamps: 9.6 k cycles for the 36 loads of a fused y / z block).
    if (SLAB && !FUSE) fuse = false;
    const bool fr = SLAB ? fuse : fro;                           // the input vector is r + beta x (wave-uniform)
    // higher-order passes of undivided meshes touch up to eleven arrays per cell: 32-bit byte offsets from the wave-uniform bases (ldo / sto)
    constexpr bool O32 = (NB > 0 && !SLAB) || FULL;
    const unsigned ob8 = (unsigned)(base * 8), sl8 = (unsigned)(sl * 8);
    unsigned tb8 = 0;                                            // DICT: byte offset of this column's row in the table
    if constexpr (STAGE) tb8 = valid ? (unsigned)sg->id * (unsigned)ld.pitch * 8u : 0u;
    else if (DICT) tb8 = valid ? (unsigned)ld.id[lineid] * (unsigned)ld.pitch * 8u : 0u;
#define NF_A8(c) (ob8 + (unsigned)(c) * sl8)
#define NF_T8(c) (tb8 + (unsigned)(c) * 8u)
    double rv[(SLAB && !FUSE) ? 1 : SEG + 1], sv[FUSE ? SEG : 1];   // r of the same cells; slab fuse: x_sol of the owned cells
    double qv[(SR && FUSE) ? SEG + 1 : 1], rq_[(SR && !FUSE) ? SEG : 1];      // SR: q of the same cells (endpoint pass); r of the owned cells (accumulation pass)
    double srr = 0.0, sqq = 0.0, srq = 0.0;
    double r1[NB > 0 ? SEG + 1 : 1], r2[NB > 1 ? SEG + 1 : 1], v1a[NB > 0 ? SEG + 1 : 1], v2a[NB > 1 ? SEG + 1 : 1], Dv[NB > 0 ? SEG : 1];
#pragma unroll
    for (int i = 0; i <= SEG; ++i) {
        const int c = c0 + i; const bool ok = valid && ((FULL && i < SEG) || c < n);
        const long a = base + (long)c * sl;
        // the overlap cell (i == SEG) is the next segment's first: keep that line for it (see k_schur_c on why this is not a ternary on i)
        if constexpr (STAGE) { const double v = sg->buf[((FULL && i < SEG) || c < n ? c : n - 1) * TX + ixl]; xv[i] = ok ? v : 0.0; }   // staged image (rows past the line were not copied)
        else if (O32) xv[i] = ok ? ldo<NT>(x, NF_A8(c)) : 0.0;
        else if (i < SEG || XC) xv[i] = ok ? ldg<NT>(x + a) : 0.0; else xv[i] = ok ? x[a] : 0.0;
        if (!SLAB || FUSE) rv[(SLAB && !FUSE) ? 0 : i] = (fr && ok) ? (SLAB ? fz.r[a] : (O32 ? ldo<NT>(x + roff, NF_A8(c)) : ldg<NT>(x + a + roff))) : 0.0;
        if (FUSE && i < SEG) sv[FUSE ? i : 0] = (fuse && ok) ? fz.xsol[a] : 0.0;
        if (SR && FUSE) qv[(SR && FUSE) ? i : 0] = (fuse && ok) ? sa.sr_q[a] : 0.0;
        if (DICT) { Lv[i] = ok ? ldo<false>(L, NF_T8(c)) : 0.0; if (i < SEG) Rv[i] = ok ? ldo<false>(DR, NF_T8(c)) : 0.0; }
        else if (O32) { Lv[i] = ok ? ldo<NT>(L, NF_A8(c)) : 0.0; if (i < SEG) Rv[i] = ok ? ldo<NT>(DR, NF_A8(c)) : 0.0; }
        else {
            if (i < SEG) Lv[i] = ok ? ldg<NT>(L + a) : 0.0; else Lv[i] = ok ? L[a] : 0.0;
            if (i < SEG) Rv[i] = ok ? ldg<NT>(DR + a) : 0.0;
        }
        if (NB > 0 && O32) {
            v1a[i] = ok ? ldo<XC>(ma.x[1], NF_A8(c)) : 0.0;
            if (NB > 1) v2a[NB > 1 ? i : 0] = ok ? ldo<XC>(ma.x[2], NF_A8(c)) : 0.0;
            r1[i] = (fro && ok) ? ldo<XC>(ma.x[1] + roff, NF_A8(c)) : 0.0;
            if (NB > 1) r2[NB > 1 ? i : 0] = (fro && ok) ? ldo<XC>(ma.x[2] + roff, NF_A8(c)) : 0.0;
            if (i < SEG) Dv[i] = ok ? ldo<false>(ma.D, NF_A8(c)) : 0.0;
        } else if (NB > 0) {
            v1a[i] = ok ? ldg<XC>(ma.x[1] + a) : 0.0;
            if (NB > 1) v2a[NB > 1 ? i : 0] = ok ? ldg<XC>(ma.x[2] + a) : 0.0;
            r1[i] = (!SLAB && fro && ok) ? ldg<XC>(ma.x[1] + a + roff) : 0.0;
            if (NB > 1) r2[NB > 1 ? i : 0] = (!SLAB && fro && ok) ? ldg<XC>(ma.x[2] + a + roff) : 0.0;
            if (i < SEG) Dv[i] = ok ? ma.D[a] : 0.0;
        }
    }
    double dinv_s = 0.0;
    if (DICT) { if (FULL || (valid && c0 < n)) dinv_s = c0 == 0 ? D0[lineid] : ldo<false>(DR, NF_T8(c0 - 1)); }
    else if (valid && c0 < n) dinv_s = c0 == 0 ? D0[lineid] : DR[base + (long)(c0 - 1) * sl];
    NF_STAMP(stamp, 3);
    if (mid(f_alpha, f_beta)) return 0.0;                        // e.g. the reduction that yields beta: runs with the loads above in flight
    // ---- arithmetic on the loaded values (cells outside the line hold zeros throughout)
#pragma unroll
    for (int i = 0; i <= SEG; ++i) {
        const int c = c0 + i; const bool ok = valid && c < n;
        if ((!SLAB || FUSE) && fr) {
            if (SR && FUSE) rv[(SLAB && !FUSE) ? 0 : i] = fma(-f_alpha, qv[(SR && FUSE) ? i : 0], rv[(SLAB && !FUSE) ? 0 : i]);   // r -= alpha q (src/solvers.cpp:610)
            if (FUSE && i < SEG) sv[FUSE ? i : 0] = fma(f_alpha, xv[i], sv[FUSE ? i : 0]);   // owned cell; the overlap cell (i == SEG) belongs to the next segment
            xv[i] = fma(f_beta, xv[i], rv[(SLAB && !FUSE) ? 0 : i]);
        }
        if (SR && FUSE && i < SEG) { const double rn = fr ? rv[(SLAB && !FUSE) ? 0 : i] : xv[i]; srr += ok ? rn * rn : 0.0; }   // |r|^2 of the owned cells (first iteration: p = r)
        if (SLAB && valid && c == n) xv[i] = x_after;
        if (NB > 0) {
            double v1 = v1a[i], v2 = NB > 1 ? v2a[NB > 1 ? i : 0] : 0.0;
            if (!SLAB && fro) { v1 = fma(f_beta, v1, r1[i]); if (NB > 1) v2 = fma(f_beta, v2, r2[NB > 1 ? i : 0]); }
            if (i < SEG) {
                x1[i] = v1; if (NB > 1) x2[NB > 1 ? i : 0] = v2;
                // cell coordinates for 1/c_e = D / factor_dir
                int cx = ix, cy = 0, cz = 0;
                if (DIR == 1) { cy = c; cz = by; } else { cy = by; cz = c + ((SLAB && sa.if_lo) ? 1 : 0); }   // chain cell c is local cell fs + c
                icv[i] = ok ? Dv[i] / geom_factor(G, DIR, cx, cy, cz) : 0.0;
            } else {
                xLn = xv[i] + ma.eL[0] * ma.Gc[0] * v1 + (NB > 1 ? ma.eL[1] * ma.Gc[1] * v2 : 0.0);
                if (SLAB && valid && c == n) xLn = x_after;          // the cell above the chain is the upper edge cell (xL, separator folded in)
            }
        }
    }
    if (FUSE && fuse) {                                    // x_sol += alpha p of the owned cells
#pragma unroll
        for (int i = 0; i < SEG; ++i) if (valid && c0 + i < n) fz.xsol[base + (long)(c0 + i) * sl] = sv[FUSE ? i : 0];
    }
    double t[NB > 0 ? SEG : 1];                                  // NB == 0: t_i = xv_i - xv_{i+1} is recomputed where needed (registers)
    double P = 1.0, lz = 0.0;
    double xL0 = xv[0];                                          // xL of this segment's first cell
    if (NB == 0) {
        (void)t;
    } else {
        double xLc[SEG + 1], xRc[SEG];
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const double g1 = ma.Gc[0] * x1[i], g2 = NB > 1 ? ma.Gc[1] * x2[i] : 0.0;
            xLc[i] = xv[i] + ma.eL[0] * g1 + (NB > 1 ? ma.eL[1] * g2 : 0.0);
            xRc[i] = xv[i] - ma.eR[0] * g1 - (NB > 1 ? ma.eR[1] * g2 : 0.0);
        }
        xLc[SEG] = xLn; xL0 = xLc[0];
#pragma unroll
        for (int i = 0; i < SEG; ++i) t[i] = xRc[i] - xLc[i + 1];
    }
#pragma unroll
    for (int i = 0; i < SEG; ++i) { const double ti = NB == 0 ? xv[i] - xv[i + 1] : t[NB > 0 ? i : 0]; lz = ti - Lv[i] * lz; P = -Lv[i] * P; }
    NF_STAMP(stamp, 4);
    if (act) { sA[si] = P; sB[si] = lz; }
    if (act && seg == 0) sZ0[ixl] = x_before - xL0;
    if constexpr (STAGE) {
        // 1/d is first used behind the barrier: with a copy in flight the compiler waits there for EVERYTHING outstanding, the copy included
        // (it cannot count across the copy loop).  Ask for the table values here, where nothing else is in flight yet.
#pragma unroll
        for (int i = 0; i < SEG; ++i) asm volatile("" :: "v"(Rv[i]));
        asm volatile("" :: "v"(dinv_s));
    }
    block_bar<STAGE>();
    NF_STAMP(stamp, 5);
    // every thread holds its x in registers and the buffer is free: the next tile's copy flies during the rest of this tile
    if constexpr (STAGE && NF_STAGE_PLACE == 0) { if (sg->next) { stage_issue<NT, FULL>(sg->buf, sg->next, n, sl, TX); sg->id = sg->next_id[ixl]; } }
    if (wscan) {
        // forward: incoming value of segment s = (f_{s-1} o ... o f_0)(z0); inclusive Hillis-Steele over the lanes of a column
        int W = 16; while (W < NSEG) W <<= 1;
        const int lane = tid & 63, cw = 64 / W, s_ = lane & (W - 1);
        if (tid < T)
            for (int c = (tid >> 6) * cw + lane / W; c < TX; c += (T >> 6) * cw) {
                double A = s_ < NSEG ? sA[c * NSP + s_] : 1.0, B = s_ < NSEG ? sB[c * NSP + s_] : 0.0;
                for (int d = 1; d < W; d <<= 1) {
                    const double Ap = __shfl_up(A, d, W), Bp = __shfl_up(B, d, W);
                    if (s_ >= d) { B = A * Bp + B; A = A * Ap; }
                }
                const double Ae = __shfl_up(A, 1, W), Be = __shfl_up(B, 1, W), z0 = sZ0[c];
                if (s_ < NSEG) sB[c * NSP + s_] = s_ == 0 ? z0 : Ae * z0 + Be;
            }
        block_bar<STAGE>();
    }
    if (SLAB && fuse && valid) {                                 // every read of the old p in this block is behind the barrier
#pragma unroll
        for (int i = 0; i < SEG; ++i) if (c0 + i < n) fz.p[base + (long)(c0 + i) * sl] = xv[i];
        if (seg == 0) { if (sa.if_lo) fz.p[edge_lo] = xe_lo; if (sa.if_hi) fz.p[edge_hi] = xe_hi; }
        if (SR && FUSE) {                                          // the updated residual: other threads of the block read the old one above (overlap and edge cells)
#pragma unroll
            for (int i = 0; i < SEG; ++i) if (c0 + i < n) sa.sr_r[base + (long)(c0 + i) * sl] = rv[(SLAB && !FUSE) ? 0 : i];
            // edge cells: every thread of the column formed r - alpha q for its p above; the owner (segment 0) forms it once more here,
            // behind the barrier, rather than keeping it alive across the scans -- the old r and q are still in place, it is their only writer
            if (seg == 0) {
                if (sa.if_lo) { const double re = fma(-f_alpha, sa.sr_q[edge_lo], fz.r[edge_lo]); sa.sr_r[edge_lo] = re; srr += re * re; }
                if (sa.if_hi) { const double re = fma(-f_alpha, sa.sr_q[edge_hi], fz.r[edge_hi]); sa.sr_r[edge_hi] = re; srr += re * re; }
            }
        }
    }
    if (SR && FUSE && !fuse && valid && seg == 0) {                // first iteration: r = p, untouched
        if (sa.if_lo) { const double re = x[edge_lo]; srr += re * re; }
        if (sa.if_hi) { const double re = x[edge_hi]; srr += re * re; }
    }
    double z;
    if (wscan) z = sB[si];
    else { z = sZ0[ixl]; for (int s = 0; s < seg; ++s) z = sA[s * TX + ixl] * z + sB[s * TX + ixl]; }
    const double zin = z;
    double w[SEG];
    double zw = (ZW && c0 == 0) ? zin * (zin * dinv_s) : 0.0;    // the line's first face (lanes outside the mesh hold zeros)
#pragma unroll
    for (int i = 0; i < SEG; ++i) { const double ti = NB == 0 ? xv[i] - xv[i + 1] : t[NB > 0 ? i : 0]; z = ti - Lv[i] * z; w[i] = z * Rv[i]; if (ZW) zw += z * w[i]; }
    if (ZW) asm volatile("" : "+v"(zw));                         // summed here, not sunk to the end of the kernel (which would keep every z alive)
    double Q = 1.0, lu = 0.0;
#pragma unroll
    for (int i = SEG - 1; i >= 0; --i) { lu = w[i] - Lv[i + 1] * lu; Q = -Lv[i + 1] * Q; }
    if (act) { sA2[si] = Q; sB2[si] = lu; }
    // y is only needed by the output stage: issue its loads here so they fly during the barrier + backward scan
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        const int c = c0 + i; const bool ok = acc && (FULL || (valid && c < n && wr));
        yo[i] = ok ? (O32 ? ldo<NT>(y, NF_A8(c)) : ldg<NT>(y + base + (long)c * sl)) : 0.0;
        if (SLAB && NB == 0 && sa.yadd) yo[i] += ok ? sa.yadd[base + (long)c * sl] : 0.0;     // same order on every cell: (y_x + y_y) + z part
    }
    double y1o[NB > 0 ? SEG : 1], y2o[NB > 1 ? SEG : 1];
    if (NB > 0) {
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const bool okl = acc && valid && c0 + i < n && wr; const long a = base + (long)(c0 + i) * sl;
            y1o[i] = okl ? (O32 ? ldo<false>(ma.y[1], NF_A8(c0 + i)) : ma.y[1][a]) : 0.0;
            if (NB > 1) y2o[NB > 1 ? i : 0] = okl ? (O32 ? ldo<false>(ma.y[2], NF_A8(c0 + i)) : ma.y[2][a]) : 0.0;
        }
    }
    if constexpr (STAGE && NF_STAGE_PLACE == 1) { if (sg->next) { stage_issue<NT, FULL>(sg->buf, sg->next, n, sl, TX); sg->id = sg->next_id[ixl]; } }   // this tile's y first in the queue
    NF_STAMP(stamp, 6);
    block_bar<STAGE>();
    NF_STAMP(stamp, 7);
    if (SR && !FUSE) {                                             // r of the owned cells (for r.q): asked for behind the barrier, so that it is not alive across
#pragma unroll                                                   // the scans (the pass sits at 128 VGPRs = four blocks of 256 threads per CU); it flies during the backward replay
        for (int i = 0; i < SEG; ++i) rq_[(SR && !FUSE) ? i : 0] = (valid && c0 + i < n && wr) ? sa.sr_r[base + (long)(c0 + i) * sl] : 0.0;
    }
    double u = 0.0;
    if (wscan) {
        // backward: incoming value of segment s = (f_{s+1} o ... o f_{NSEG-1})(0) = the B part of the suffix composition at s + 1
        int W = 16; while (W < NSEG) W <<= 1;
        const int lane = tid & 63, cw = 64 / W, s_ = lane & (W - 1);
        if (tid < T)
            for (int c = (tid >> 6) * cw + lane / W; c < TX; c += (T >> 6) * cw) {
                double A = s_ < NSEG ? sA2[c * NSP + s_] : 1.0, B = s_ < NSEG ? sB2[c * NSP + s_] : 0.0;
                for (int d = 1; d < W; d <<= 1) {
                    const double Ap = __shfl_down(A, d, W), Bp = __shfl_down(B, d, W);
                    if (s_ + d < W) { B = A * Bp + B; A = A * Ap; }
                }
                const double Bn = __shfl_down(B, 1, W);
                if (s_ < NSEG) sA2[c * NSP + s_] = s_ == W - 1 ? 0.0 : Bn;
            }
        block_bar<STAGE>();
        if (act) u = sA2[si];
    } else if (act) for (int s = NSEG - 1; s > seg; --s) u = sA2[s * TX + ixl] * u + sB2[s * TX + ixl];
#pragma unroll
    for (int i = SEG - 1; i >= 0; --i) { u = w[i] - Lv[i + 1] * u; w[i] = u; }
    const double ulo = zin * dinv_s - Lv[0] * w[0];             // u at the lower face of this segment
    double dot = 0.0;
    if (wr) {
        // values first, branch-free (cells outside the line contribute exact zeros), then the stores: a store inside a predicated
        // region that also uses loaded data would wait for the previous cell's store to be acknowledged (vmcnt counts stores too)
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const double lo = i == 0 ? ulo : w[i > 0 ? i - 1 : 0];
            const bool in = FULL || (valid && c0 + i < n);       // a select, not a branch (slab chains: xv of the cell behind the chain end is the edge cell)
            yo[i] = yo[i] + ma.Ta * (w[i] - lo);
            if constexpr (FULL && !ZW) {                         // the select below keeps product and sum apart; without it they must not fuse into an fma either
#pragma clang fp contract(off)
                dot += xv[i] * yo[i];
            } else if (!ZW) dot += in ? xv[i] * yo[i] : 0.0;
            if (SR && !FUSE) { sqq += in ? yo[i] * yo[i] : 0.0; srq += in ? rq_[(SR && !FUSE) ? i : 0] * yo[i] : 0.0; }
            if (NB > 0) {
                const double v = ma.Gc[0] * x1[i] * ma.iM[0] * icv[i] - (ma.eL[0] * lo + ma.eR[0] * w[i]);
                y1o[i] = y1o[i] + ma.Ta * ma.Gc[0] * v; dot += in ? x1[i] * y1o[i] : 0.0;
            }
            if (NB > 1) {
                const double v = ma.Gc[1] * x2[NB > 1 ? i : 0] * ma.iM[1] * icv[i] - (ma.eL[1] * lo + ma.eR[1] * w[i]);
                y2o[NB > 1 ? i : 0] = y2o[NB > 1 ? i : 0] + ma.Ta * ma.Gc[1] * v; dot += in ? x2[NB > 1 ? i : 0] * y2o[NB > 1 ? i : 0] : 0.0;
            }
        }
        if constexpr (STAGE) {
            // the values are formed HERE: in the z.w form nothing but the store uses them, and the compiler would sink each sum into its
            // store's predicated region, where it waits for every older memory operation -- the previous cell's store among them
#pragma unroll
            for (int i = 0; i < SEG; ++i) asm volatile("" : "+v"(yo[i]));
            asm volatile("" : "+v"(sg->id));                       // the next tile's table row too: asked for here, not behind the stores
            // y is here, and with it everything older: this wave's part of the next tile's copy has landed.  Said by hand, because the
            // top of the next tile relies on it and does not wait again -- the stores below drain under the next tile's table loads
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const int c = c0 + i;
            if (FULL || (valid && c < n)) {
                const long a = base + (long)c * sl;
                if (FULL) sto(y, NF_A8(c), yo[i]);
                else if (O32) {
                    sto(y, NF_A8(c), yo[i]); sto(ma.y[1], NF_A8(c), y1o[i]);
                    if (NB > 1) sto(ma.y[2], NF_A8(c), y2o[NB > 1 ? i : 0]);
                } else {
                    y[a] = yo[i];
                    if (NB > 0) ma.y[1][a] = y1o[i];
                    if (NB > 1) ma.y[2][a] = y2o[NB > 1 ? i : 0];
                }
            }
        }
    }
    if (ZW) dot = ma.Ta * zw;
    if (SLAB && sa.mode == 3) {                                 // emit J_z = -u on every face of the local line (+ the z bubbles for RT1+)
        if (valid) {
            const long nxy = sl;                                 // z lines: stride between planes = nx * ny
            int am = 0;                                          // sa.amode[bz] without a dynamic index (that would put the whole argument struct in scratch)
#pragma unroll
            for (int m = 0; m < 9; ++m) if ((unsigned)m == bz) am = sa.amode[m];
            const int fs = sa.if_lo ? 1 : 0, nfa = sa.nfa, kb = G.k, ni_ = sa.ni;
            double *const jz_ = sa.jz, *const jzb_ = sa.jzb;     // locals: a lambda that captured `sa` itself would force the argument struct into scratch
            const double eL0 = ma.eL[0], eL1 = ma.eL[1], eR0 = ma.eR[0], eR1 = ma.eR[1], Gc0 = ma.Gc[0], Gc1 = ma.Gc[1], iM0 = ma.iM[0], iM1 = ma.iM[1];
            auto face = [=](long fpl) -> double & { return jz_[(fpl * nxy + lineid) * nfa + am]; };
            // bubbles of a cell between face values (lo, hi): v_l = G_l x_{l+1} iM_l / c_e - (eL_l lo + eR_l hi); inactive ones (l >= NB) have no source
            auto bubbles = [=](long cell, double lo, double hi, double xb1, double xb2, double ice) {
                for (int l = 0; l < kb; ++l) {
                    const double xb = l == 0 ? xb1 : xb2, Gl = l == 0 ? Gc0 : Gc1, iMl = l == 0 ? iM0 : iM1, eLl = l == 0 ? eL0 : eL1, eRl = l == 0 ? eR0 : eR1;
                    const double tb = l < NB ? Gl * xb * iMl * ice : 0.0;
                    jzb_[cell * ni_ + l + kb * am] = -(tb - (eLl * lo + eRl * hi));
                }
            };
#pragma unroll
            for (int i = 0; i < SEG; ++i) if (c0 + i < n) {
                face(fs + c0 + i + 1) = -w[i];
                if (kb > 0) bubbles((long)(fs + c0 + i) * nxy + lineid, i == 0 ? ulo : w[i > 0 ? i - 1 : 0], w[i], NB > 0 ? x1[NB > 0 ? i : 0] : 0.0, NB > 1 ? x2[NB > 1 ? i : 0] : 0.0,
                                    NB > 0 ? icv[NB > 0 ? i : 0] : 0.0);
            }
            if (seg == 0) {
                face(fs) = -ulo;                                 // lower face of the first chain cell
                if (sa.if_lo) {
                    const double us = sa.ulo[lm];
                    face(0) = -us;                               // the separator below
                    if (kb > 0) bubbles(lineid, us, ulo, NB > 0 ? ma.x[NB > 0 ? 1 : 0][edge_lo] : 0.0, NB > 1 ? ma.x[NB > 1 ? 2 : 0][edge_lo] : 0.0,
                                        NB > 0 ? ma.D[edge_lo] / geom_factor(G, DIR, ix, (int)by, 0) : 0.0);
                }
            }
            if (sa.if_hi && c0 <= n - 1 && n - 1 < c0 + SEG) {     // the thread that owns the last chain cell: separator above + upper edge cell
                double ulast = 0.0;
#pragma unroll
                for (int i = 0; i < SEG; ++i) if (c0 + i == n - 1) ulast = w[i];
                const double us = sa.uhi[lm];
                face(fs + n + 1) = -us;
                if (kb > 0) bubbles((long)(fs + n) * nxy + lineid, ulast, us, NB > 0 ? ma.x[NB > 0 ? 1 : 0][edge_hi] : 0.0, NB > 1 ? ma.x[NB > 1 ? 2 : 0][edge_hi] : 0.0,
                                    NB > 0 ? ma.D[edge_hi] / geom_factor(G, DIR, ix, (int)by, fs + n) : 0.0);
            }
        }
        return 0.0;
    }
    if (SLAB) {
        // chain end values: u_first by the segment-0 thread, u_last by the thread owning chain cell n-1
        // (edge values are re-read here instead of being kept live across the two scans: x holds the updated p by now, and the
        // per-line coefficients come from L2 -- the kernel sits at the 128-VGPR limit of a 1024-thread block)
        if (valid && seg == 0 && sa.if_lo) {
            const double a_lo = sa.alo[lineid];
            if (sa.mode == 1) sa.clo[lm] = -(NB == 0 ? x[edge_lo] : xe_lo) - a_lo * ulo;
            else {
                const double u_lo = sa.fold ? (sa.rlo[lm] + sa.clo[lm]) * sa.sinv_lo[lineid] : sa.ulo[lm];
                const double xe = x[edge_lo]; const double yv = (y[edge_lo] + ((NB == 0 && sa.yadd) ? sa.yadd[edge_lo] : 0.0)) + ma.Ta * (ulo - u_lo); y[edge_lo] = yv; dot += xe * yv;
                if (SR && !FUSE) { sqq += yv * yv; srq += sa.sr_r[edge_lo] * yv; }
                if (NB > 0) {                                    // bubbles of the edge cell: faces (separator, first chain face)
                    const double ice = ma.D[edge_lo] / geom_factor(G, DIR, ix, (int)by, 0);
#pragma unroll
                    for (int l = 0; l < NB; ++l) {
                        const double xb = ma.x[l + 1][edge_lo];
                        const double v = ma.Gc[l] * xb * ma.iM[l] * ice - (ma.eL[l] * u_lo + ma.eR[l] * ulo);
                        const double yb = ma.y[l + 1][edge_lo] + ma.Ta * ma.Gc[l] * v;
                        ma.y[l + 1][edge_lo] = yb; dot += xb * yb;
                    }
                }
            }
        }
        if (valid && sa.if_hi && c0 <= n - 1 && n - 1 < c0 + SEG) {
            double ulast = 0.0;
#pragma unroll
            for (int i = 0; i < SEG; ++i) if (c0 + i == n - 1) ulast = w[i];
            const double a_hi = sa.ahi[lineid];
            if (sa.mode == 1) sa.chi[lm] = (NB == 0 ? x[edge_hi] : xe_hi) - a_hi * ulast;
            else {
                const double u_hi = sa.fold ? (sa.chi[lm] + sa.rhi[lm]) * sa.sinv_hi[lineid] : sa.uhi[lm];
                const double xe = x[edge_hi]; const double yv = (y[edge_hi] + ((NB == 0 && sa.yadd) ? sa.yadd[edge_hi] : 0.0)) + ma.Ta * (u_hi - ulast); y[edge_hi] = yv; dot += xe * yv;
                if (SR && !FUSE) { sqq += yv * yv; srq += sa.sr_r[edge_hi] * yv; }
                if (NB > 0) {                                    // faces (last chain face, separator)
                    const int fsz = sa.if_lo ? 1 : 0;
                    const double ice = ma.D[edge_hi] / geom_factor(G, DIR, ix, (int)by, fsz + n);
#pragma unroll
                    for (int l = 0; l < NB; ++l) {
                        const double xb = ma.x[l + 1][edge_hi];
                        const double v = ma.Gc[l] * xb * ma.iM[l] * ice - (ma.eL[l] * ulast + ma.eR[l] * u_hi);
                        const double yb = ma.y[l + 1][edge_hi] + ma.Ta * ma.Gc[l] * v;
                        ma.y[l + 1][edge_hi] = yb; dot += xb * yb;
                    }
                }
            }
        }
    }
    if (SR && FUSE) return srr;                                    // endpoint pass: this thread's share of |r|^2
    if (SR && extra) { extra[0] = sqq; extra[1] = srq; }
    return dot;
#undef NF_A8
#undef NF_T8
}

// Slab variants keep r and x_sol of their cells in registers next to x, L, 1/d (loads first, see schur_s_tile): blocks of at most 512
// threads, so that the register budget is 256 per thread (the host picks TX accordingly)
struct StageGrid { unsigned gx = 0, gy = 0; };                  // SV_STAGE: the tile grid that a persistent launch walks (gridDim holds the block count)
template <int SEG, int DIR, bool SLAB, int NB, unsigned V = 0, int FULL = 0>   // FULL: the staged pass on a grid of whole tiles, see schur_s_tile
__global__ __launch_bounds__(SLAB ? 512 : 1024, SLAB ? (NB > 0 ? 2 : ((V & SV_FUSE) ? ((V & SV_SR) ? NF_SR_Z1_WAVES : 3) : ((V & SV_SR) ? NF_SR_Z2_WAVES : 4))) : 1) void k_schur_s(ModeArgs ma0, ModeTab mt, Geom G, const double *__restrict__ L, const double *__restrict__ DR,
                          const double *__restrict__ D0, int n, long sl, long outer_stride, int nx, int TX, int NSEG,
                          int last, double *__restrict__ partials, const CgScalars *__restrict__ cg, SlabArgs sa, CgFuse fz, CgLean lean,
                          LineDict ld = LineDict(), StageGrid sgr = StageGrid())
{
    static_assert(schur_s_legal(SEG, DIR, SLAB, NB, V), "not a variant of k_schur_s");
    static_assert(FULL == 0 || (FULL == 1 && (V & SV_STAGE)), "whole-tile form: the staged pass");
    constexpr bool FUSE = V & SV_FUSE, SR = V & SV_SR;
    extern __shared__ double sm[];
    if (cg && cg->done) return;
    if constexpr (V & SV_STAGE) {
        // Persistent form: gridDim.x blocks walk the gx * gy tiles, block b takes b, b + gridDim.x, ...  A tile's (bx, by) and its slot in
        // `partials` are what the one-tile-per-block launch derives from blockIdx (the XCD-contiguous order included), so the first-stage
        // sums land where they land there.  Every barrier between a copy's issue and the wait at the top of the next tile is the raw one.
        const ModeArgs ma = select_mode(ma0, mt, blockIdx.z, NB + 1);
        double *sred = sm + 4 * TX * (NSEG + 1) + TX;
        const double *buf = sred + 32;                            // behind the summary arrays and the reduction scratch (SegPlan::lds)
        const unsigned gx = sgr.gx, gy = sgr.gy, tiles = gx * gy;
        const bool remap = sa.xcd && tiles % 8 == 0;
        auto origin = [&](unsigned t, unsigned &bx, unsigned &by) {
            const unsigned nl = remap ? (t % 8) * (tiles / 8) + t / 8 : t;
            bx = nl % gx; by = nl / gx;
        };
        auto tile_x = [&](unsigned t) { unsigned bx, by; origin(t, bx, by); return ma.x[0] + ((long)by * outer_stride + (long)bx * TX); };
        auto tile_id = [&](unsigned t) { unsigned bx, by; origin(t, bx, by); return ld.id + ((long)by * nx + (long)bx * TX); };
        const int ixl0 = (int)threadIdx.x < TX * NSEG ? (int)threadIdx.x % TX : 0;   // schur_s_tile's ixl
        unsigned t = blockIdx.x;
        StageCtx sg; sg.buf = buf;
        if (t < tiles) { stage_issue<(V & SV_NT) != 0>(buf, tile_x(t), n, sl, TX); sg.id = tile_id(t)[ixl0]; }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the first tile's copy; the later ones are waited for inside the tile before
        asm volatile("" : "+v"(sg.id));                           // (the compiler's own wait for the table row: here, not behind a tile's stores)
        for (; t < tiles; t += gridDim.x) {
            unsigned bx, by; origin(t, bx, by);
            const bool more = t + gridDim.x < tiles;
            sg.next = more ? tile_x(t + gridDim.x) : nullptr; sg.next_id = more ? tile_id(t + gridDim.x) : nullptr;
            // the copy of this tile has landed: every issuing wave has seen its counter drain, and here the block meets
            block_bar<true>();
            const double dot = schur_s_tile<SEG, DIR, SLAB, NB, V, NoMid, false, FULL != 0>(ma, G, L, DR, D0, n, sl, outer_stride, nx, TX, NSEG, bx, by, blockIdx.z, gy,
                                                                    (int)threadIdx.x, true, sm, sa, fz, false, false, 0.0, 0.0, !sa.noacc,
                                                                    nullptr, NoMid(), nullptr, ld, &sg);
            if (last && partials) {
                const double s = block_sum<true>(dot, sred);
                if (threadIdx.x == 0) partials[((long)blockIdx.z * gy + by) * gx + bx] = s;
            }
        }
        return;
    }
    const ModeArgs ma = select_mode(ma0, mt, blockIdx.z, NB + 1);
    // fused CG on slabs: the endpoint pass (mode 1) is the first to read p in an iteration, so it carries the deferred
    // x_sol += alpha p, p = r + beta p (see CgFuse); every cell of the local line is owned by exactly one thread.
    // With lean.st it is also the consumer of the all-reduced |r|^2 (FIN_RR: beta, stop tests), like the x pass of an undivided mesh.
    bool fuse = FUSE && sa.mode == 1 && fz.p != nullptr && (SR ? sa.sr.index > 0 : (lean.st ? !lean.first : cg->its > 0));
    double f_beta = fuse && !lean.st && !SR ? cg->beta : 0.0;
    if (SLAB && !SR && lean.st && !lean.first) {
        double *sred_l = sm + 4 * TX * (NSEG + 1) + TX;
        if (lean_rr_step(lean, blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0, sred_l, &f_beta)) return;
    }
    double f_alpha = fuse && !SR ? cg->alpha : 0.0;
    // single-reduction CG: every block derives alpha, beta and the stop decision from the same five all-reduced doubles (see Cg1)
    if (SR && FUSE && fuse) { if (cg1_step(sa.sr, blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0, &f_alpha, &f_beta)) return; }
    // XCD-aware tile order (experiment, sa.xcd): hardware deals consecutive workgroups round-robin to the 8 XCDs; remap so that
    // each XCD works on one contiguous range of tiles
    unsigned bx = blockIdx.x, by = blockIdx.y;
    if (sa.xcd) {
        const unsigned nblk = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
        if (nblk % 8 == 0) { const unsigned nl = (lin % 8) * (nblk / 8) + lin / 8; bx = nl % gridDim.x; by = nl / gridDim.x; }
    }
    double extra[2] = { 0.0, 0.0 };                              // (the staged variants have returned above: the whole-tile body is not instantiated here)
    const double dot = schur_s_tile<SEG, DIR, SLAB, NB, V, NoMid, false, false>(ma, G, L, DR, D0, n, sl, outer_stride, nx, TX, NSEG, bx, by, blockIdx.z, gridDim.y,
                                                            (int)threadIdx.x, true, sm, sa, fz, fuse, false, f_alpha, f_beta, !(!SLAB && NB == 0 && sa.noacc),
                                                            nullptr, NoMid(), SR ? extra : nullptr, ld);
    if (SLAB && sa.mode == 3) return;
    double *sred = sm + 4 * TX * (NSEG + 1) + TX;
    const long pidx = ((long)blockIdx.z * gridDim.y + by) * gridDim.x + bx;
    if (SR && FUSE) {                                            // endpoint pass: |r|^2 of the residual this iteration starts with
        const double s = block_sum(dot, sred);
        if (threadIdx.x == 0) sa.sr_part[pidx] = s;
        return;
    }
    if (last && partials) {
        if (SR) {                                                // accumulation pass: q.q and r.q next to p.q (24 doubles of reduction scratch: blocks of at most 512 threads)
            double s0 = dot, s1 = extra[0], s2 = extra[1];
            block_sum3(s0, s1, s2, sred);
            if (threadIdx.x == 0) { partials[pidx] = s0; partials[pidx + sa.sr_stride] = s1; partials[pidx + 2 * sa.sr_stride] = s2; }
        } else {
            const double s = block_sum(dot, sred);
            if (threadIdx.x == 0) partials[pidx] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The endpoint pass of the z lines WITHOUT a line solve (single-reduction CG on RT0-P0 slab teams).  What the partition method needs from
// the first chain solve of an apply are two numbers per z line: c_lo = -x_edge - a_lo u_first and c_hi = x_edge - a_hi u_last, with
// u = T^-1 t(x).  Both are LINEAR functionals of the line's cell values, c_lo = sum_k W_lo[k] x_k, c_hi = sum_k W_hi[k] x_k, and their weights
// depend on the factored operator only: the host measures them once per BuildMatrices by sending the unit vector of every plane through the
// endpoint pass itself (team_endpoint_weights: nz launches per group; |W_lo[k]| decays like 0.268^k away from its interface).  The pass then is
// a streaming kernel -- the deferred CG update of every cell (r -= alpha q, x += alpha p, p = r + beta p: the same fma expressions as the scan
// kernel's) and two multiply-adds per cell -- with no scan, no segment summaries and one barrier; on the 2 M-cell slabs of a strong-scaling run,
// where the scan kernel is latency-bound, that is 41 -> 30 us per launch for the same bytes (72 B per cell: W_lo, W_hi replace L, 1/d).
// Thread = (x column, one of four z ranges); the four partial sums of a line are added in a fixed order.
__global__ __launch_bounds__(256) void k_endpoint_w(double *__restrict__ p, double *__restrict__ r, const double *__restrict__ q, double *__restrict__ xsol,
                                                    const double *__restrict__ Wlo, const double *__restrict__ Whi, double *__restrict__ clo,
                                                    double *__restrict__ chi, int nx, int ny, int nz, int if_lo, int if_hi, int kcut, Cg1 sr,
                                                    const CgScalars *__restrict__ cg, double *__restrict__ rr_part)
{
    __shared__ double s_lo[4][64], s_hi[4][64], sred[4];
    if (cg && cg->done) return;
    double alpha = 0.0, beta = 0.0;
    const bool upd = sr.index > 0;
    if (upd && cg1_step(sr, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0, &alpha, &beta)) return;   // every block: the same five doubles, the same decision
    const int ixl = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int ix = blockIdx.x * 64 + ixl;
    const bool valid = ix < nx;
    const long nxy = (long)nx * ny, line = (long)blockIdx.y * nx + ix;
    const int per = (nz + 3) >> 2, k0 = seg * per, k1 = k0 + per < nz ? k0 + per : nz;
    double a_lo = 0.0, a_hi = 0.0, rr = 0.0;
    if (valid) {
#pragma unroll 4
        for (int k = k0; k < k1; ++k) {
            const long e = (long)k * nxy + line;
            double pv = p[e];
            if (upd) {
                const double rv = fma(-alpha, q[e], r[e]);           // src/solvers.cpp:610
                xsol[e] = fma(alpha, pv, xsol[e]);                   // :609
                pv = fma(beta, pv, rv);                              // :630
                r[e] = rv; p[e] = pv; rr += rv * rv;
            } else rr += pv * pv;                                    // first iteration: p = r
            // |W_lo[k]| <= 0.268^k |W_lo[0]| whatever the cross sections (T is a sum of cell blocks a_c [[2,1],[1,2]]: Jacobi-scaled condition <= 3), so
            // beyond kcut = 40 planes from its interface a weight is below 1e-22 of the sum: thick slabs do not read it (wave-uniform branch)
            if (if_lo && k < kcut) a_lo = fma(Wlo[e], pv, a_lo);
            if (if_hi && k >= nz - kcut) a_hi = fma(Whi[e], pv, a_hi);
        }
    }
    s_lo[seg][ixl] = a_lo; s_hi[seg][ixl] = a_hi;
    __syncthreads();
    if (seg == 0 && valid) {
        if (if_lo) clo[line] = ((s_lo[0][ixl] + s_lo[1][ixl]) + s_lo[2][ixl]) + s_lo[3][ixl];
        if (if_hi) chi[line] = ((s_hi[0][ixl] + s_hi[1][ixl]) + s_hi[2][ixl]) + s_hi[3][ixl];
    }
    const double s = block_sum(rr, sred);
    if (threadIdx.x == 0) rr_part[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------
// Long y / z lines (RT0-P0, plain lines: no slab interfaces).  k_schur_s holds a whole line in the registers of one block, so at
// 512 cells per line a block is only 16 columns wide (128-byte row pieces) and at 1024 cells 8 (64 bytes).  Here the line is cut
// into TWO chunks of CH = 8 NS cells and the block is twice as wide for the same number of threads:
//   forward sweep of chunk 0 (its face values w and its factors L are parked in LDS: 2 x 64 KB for 1024 threads), forward and
//   backward sweep of chunk 1 out of registers (exactly k_schur_s's body), backward sweep of chunk 0 out of LDS.
// A chunk boundary is a segment boundary like any other -- the same affine-map summaries, composed serially per thread; the z
// (u) value that crosses it is handed over through sC.  Every global array is read once and written once per pass.  The pass's
// share of x.y is formed in the forward sweeps as T_a sum z_f w_f (see schur_s_tile, ZW), so the backward half needs no x.
// LDS (doubles): sA, sB [NS TX] (forward and backward summaries in turn), sC, sL1 [TX], 16 of reduction scratch, pW, pL [CH TX], pZ [NS TX].
// Per cell the same expressions as k_schur_s (the value crossing the chunk boundary is the swept one, not a composed summary:
// the two kernels agree to rounding, not bitwise).
// Addresses are 32-bit BYTE offsets from the (wave-uniform) array bases -- the host takes this kernel only while one group's array is
// below 4 GiB.  One VGPR per cell address, shared by x, L, 1/d and y, instead of a 64-bit pair per array: that is what keeps the
// two-chunk body inside the 128 registers of a 1024-thread block (with 64-bit addresses it spilled 10-12 registers to scratch,
// +31 % bytes written and +6 % fetched per pass by the PMC counters, profiles/r03_b_pmc_512_chunked.json).
// DICT (see LineDict): L and DR point at the table of distinct lines, reached from the byte offset of the column's row; x and y stream as before.
// EARLY (table instantiations only: without L and 1/d to stream they have the registers for it): the block's own vector loads go out ahead of
// the sweeps that hide them, instead of one dependent HBM round trip per chunk and half.  1: x of chunk 1 is requested right behind chunk 0's
// loads (chunk 0 first, so that a counted wait lets its sweep start on its own data); 2: also y of chunk 1 before the barrier of chunk 1's
// forward sweep and y of chunk 0 before the first barrier of the backward half.  Same predicates, same hints, no arithmetic moves: the bits
// of y and of the dot product are those of EARLY = 0.  The tile, the grid and the LDS layout stay as they are.
// FULL (EARLY = 2 only; the host's c_full): the tile grid has no partial tile -- nx a multiple of TX, n = 16 NS, TX NS threads -- so every predicate
// on a load or a store is true at compile time but the one of the overlap cell behind the line's last segment: straight-line accesses, counted
// waits, a third fewer instructions.  Values and arithmetic are untouched.
// The instantiations: the table next to the streaming loads only; early loads (levels 1, 2) with the table only, see EARLY; FULL with EARLY = 2 only
constexpr bool schur_c_legal(int DIR, bool NT, bool DICT, int EARLY, int FULL = 0) { return (DIR == 1 || DIR == 2) && (!DICT || NT) && EARLY >= 0 && EARLY <= (DICT ? 2 : 0) && (FULL == 0 || (FULL == 1 && DICT && EARLY == 2)); }
template <int DIR, bool NT, bool DICT = false, int EARLY = 0, int FULL = 0>   // FULL: a grid of whole tiles, see below
__global__ __launch_bounds__(1024, 1) void k_schur_c(const double *__restrict__ x, double *__restrict__ y, double Ta,
                                                     const double *__restrict__ L, const double *__restrict__ DR, const double *__restrict__ D0,
                                                     int n, long sl, long outer_stride, int nx, int TX, int NS, int last,
                                                     double *__restrict__ partials, const CgScalars *__restrict__ cg, int xcd, LineDict ld = LineDict())
{
    static_assert(schur_c_legal(DIR, NT, DICT, EARLY, FULL), "not a variant of k_schur_c");
    extern __shared__ double sm[];
    if (cg && cg->done) return;
    constexpr int SEG = 8;
    const int T = TX * NS, CH = NS * SEG;
    double *sA = sm, *sB = sm + T, *sC = sm + 2 * T, *sL1 = sC + TX, *sred = sL1 + TX, *pW = sred + 16, *pL = pW + (long)CH * TX, *pZ = pL + (long)CH * TX;
    unsigned bx = blockIdx.x, by = blockIdx.y;
    if (xcd) {                                                   // XCD-contiguous tile order, as in k_schur_s
        const unsigned nblk = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
        if (nblk % 8 == 0) { const unsigned nl = (lin % 8) * (nblk / 8) + lin / 8; bx = nl % gridDim.x; by = nl / gridDim.x; }
    }
    const int tid = (int)threadIdx.x;
    const bool act = FULL || tid < T;                            // FULL (the host's c_full): one thread per (column, segment), every cell of both chunks on the line
    const int ixl = act ? tid % TX : 0, seg = act ? tid / TX : 0, si = seg * TX + ixl;
    const int ix = (int)bx * TX + ixl;
    const bool valid = FULL || (act && ix < nx);
    const unsigned slb = (unsigned)(sl * 8);                     // bytes between the cells of a line
    const unsigned ob = (unsigned)(((long)by * outer_stride + ix) * 8);   // byte offset of the line's first cell
    const long lineid = (long)by * nx + ix;
    const bool need_dot = last && partials;
    unsigned tb = 0;                                             // DICT: byte offset of this column's row in the table
    if (DICT) tb = valid ? (unsigned)ld.id[lineid] * (unsigned)ld.pitch * 8u : 0u;
    double xv[SEG + 1], Lv[SEG + 1], Rv[SEG], w[SEG], yo[SEG];
    double x1[EARLY >= 1 ? SEG + 1 : 1], y0[EARLY >= 2 ? SEG : 1];   // EARLY: x of chunk 1, y of chunk 0, in flight under the sweeps before their use
    double zin = 0.0, dinv_s = 0.0, zc = 0.0, dot = 0.0;
    // ---- forward sweeps, chunk 0 then chunk 1 (both ch loops unrolled: the early arrays must stay in registers)
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const int c0 = ch * CH + seg * SEG;
        const unsigned o0 = ob + (unsigned)c0 * slb;
#pragma unroll
        for (int i = 0; i <= SEG; ++i) {                         // loads only (see schur_s_tile)
            const bool ok = valid && ((FULL && (i < SEG || ch == 0)) || c0 + i < n);   // FULL: all but the overlap cell of the line's last segment
            const unsigned a = o0 + (unsigned)i * slb;
            // the overlap cell (i == SEG) is the next segment's first: a plain load keeps that line for it.  Two statements, not a
            // ternary on i: before the loop is unrolled a ternary is one load in each arm of a branch, which the optimiser merges
            // into a single load WITHOUT the hint (that is what round 2's kernels ran: every load of x was a plain one)
            if (DICT && EARLY >= 1 && ch == 1) {                 // x came with chunk 0's loads
                const unsigned ta = tb + (unsigned)(c0 + i) * 8u;
                xv[i] = x1[i]; Lv[i] = ok ? ldo<false>(L, ta) : 0.0;
                if (i < SEG) Rv[i] = ok ? ldo<false>(DR, ta) : 0.0;
            } else if (DICT) {
                const unsigned ta = tb + (unsigned)(c0 + i) * 8u;
                if (i < SEG) { xv[i] = ok ? ldo<NT>(x, a) : 0.0; Lv[i] = ok ? ldo<false>(L, ta) : 0.0; Rv[i] = ok ? ldo<false>(DR, ta) : 0.0; }
                else { xv[i] = ok ? ldo<false>(x, a) : 0.0; Lv[i] = ok ? ldo<false>(L, ta) : 0.0; }
            } else if (i < SEG) { xv[i] = ok ? ldo<NT>(x, a) : 0.0; Lv[i] = ok ? ldo<NT>(L, a) : 0.0; Rv[i] = ok ? ldo<NT>(DR, a) : 0.0; }
            else { xv[i] = ok ? ldo<false>(x, a) : 0.0; Lv[i] = ok ? ldo<false>(L, a) : 0.0; }
        }
        double ds = 0.0;
        if (DICT) { if (FULL || (valid && c0 < n)) ds = c0 == 0 ? D0[lineid] : ldo<false>(DR, tb + (unsigned)(c0 - 1) * 8u); }
        else if (valid && c0 < n) ds = c0 == 0 ? D0[lineid] : ldo<false>(DR, o0 - slb);
        if (EARLY >= 1 && ch == 0) {                             // chunk 1's x behind chunk 0's loads: same predicate, same hints, two statements
#pragma unroll
            for (int i = 0; i <= SEG; ++i) {
                const int c1 = CH + seg * SEG + i;
                const bool ok = valid && ((FULL && i < SEG) || c1 < n);
                const unsigned a = ob + (unsigned)c1 * slb;
                if (i < SEG) x1[i] = ok ? ldo<NT>(x, a) : 0.0;
                else x1[i] = ok ? ldo<false>(x, a) : 0.0;
            }
        }
        if (EARLY >= 2 && ch == 1) {                             // chunk 1's y: lands under this sweep, consumed by the backward one
#pragma unroll
            for (int i = 0; i < SEG; ++i) yo[i] = (FULL || (valid && c0 + i < n)) ? ldo<NT>(y, o0 + (unsigned)i * slb) : 0.0;
        }
        if (ch) __syncthreads();                                 // chunk 0's summaries and carry have been consumed
        double P = 1.0, lz = 0.0;
#pragma unroll
        for (int i = 0; i < SEG; ++i) { const double ti = xv[i] - xv[i + 1]; lz = ti - Lv[i] * lz; P = -Lv[i] * P; }
        if (act) { sA[si] = P; sB[si] = lz; }
        if (act && ch == 0 && seg == 0) sC[ixl] = -xv[0];        // z entering the line (Dirichlet / natural end: no cell below)
        if (act && ch == 1 && seg == NS - 1) sC[ixl] = zc;       // z leaving chunk 0
        if (act && ch == 1 && seg == 0) sL1[ixl] = Lv[0];        // the factor just above chunk 0 (its last segment's overlap cell)
        __syncthreads();
        double z = sC[ixl];
        for (int s = 0; s < seg; ++s) z = sA[s * TX + ixl] * z + sB[s * TX + ixl];
        zin = z; dinv_s = ds;
        if (c0 == 0) dot = zin * (zin * ds);                     // the line's first face
#pragma unroll
        for (int i = 0; i < SEG; ++i) { const double ti = xv[i] - xv[i + 1]; z = ti - Lv[i] * z; w[i] = z * Rv[i]; dot += z * w[i]; }
        asm volatile("" : "+v"(dot));                            // summed HERE: left alone, the optimiser sinks the products to the kernel's end and keeps every z and w of both chunks alive (in scratch) until then
        zc = z;
        if (ch == 0 && act) {
#pragma unroll
            for (int i = 0; i < SEG; ++i) { pW[(seg * SEG + i) * TX + ixl] = w[i]; pL[(seg * SEG + i) * TX + ixl] = Lv[i]; }
            pZ[si] = zin;
        }
    }
    // ---- backward sweeps and output, chunk 1 (still in registers) then chunk 0 (from LDS)
    double ucar = 0.0;
    if (EARLY >= 2) {                                            // chunk 0's y: lands under chunk 1's backward sweep
#pragma unroll
        for (int i = 0; i < SEG; ++i) { const int c = seg * SEG + i; y0[i] = (FULL || (valid && c < n)) ? ldo<NT>(y, ob + (unsigned)c * slb) : 0.0; }
    }
#pragma unroll
    for (int ch = 1; ch >= 0; --ch) {
        const int c0 = ch * CH + seg * SEG;
        const unsigned o0 = ob + (unsigned)c0 * slb;
        if (ch == 0) {
            // (the index is made opaque: otherwise the optimiser forwards the values this thread parked itself, i.e. keeps all of chunk 0
            // alive across chunk 1 -- in scratch memory, since the registers are full: 100 B per lane of spills instead of LDS reads)
            int pbase = seg * SEG * TX + ixl;
            asm volatile("" : "+v"(pbase));
#pragma unroll
            for (int i = 0; i < SEG; ++i) { w[i] = pW[pbase + i * TX]; Lv[i] = pL[pbase + i * TX]; }
            Lv[SEG] = seg < NS - 1 ? pL[(seg + 1) * SEG * TX + ixl] : sL1[ixl];   // written before the barriers in between
            zin = pZ[si];
            dinv_s = 0.0;
            if (DICT) { if (FULL || (valid && c0 < n)) dinv_s = c0 == 0 ? D0[lineid] : ldo<false>(DR, tb + (unsigned)(c0 - 1) * 8u); }
            else if (valid && c0 < n) dinv_s = c0 == 0 ? D0[lineid] : ldo<false>(DR, o0 - slb);
        }
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            if (EARLY < 2) yo[i] = (valid && c0 + i < n) ? ldo<NT>(y, o0 + (unsigned)i * slb) : 0.0;
            else if (ch == 0) yo[i] = y0[i];
        }
        __syncthreads();                                         // the summaries of the previous sweep have been consumed
        double Q = 1.0, lu = 0.0;
#pragma unroll
        for (int i = SEG - 1; i >= 0; --i) { lu = w[i] - Lv[i + 1] * lu; Q = -Lv[i + 1] * Q; }
        if (act) { sA[si] = Q; sB[si] = lu; }
        if (act && ch == 0 && seg == 0) sC[ixl] = ucar;          // u entering chunk 0 from above: first face value of chunk 1
        __syncthreads();
        double u = ch == 1 ? 0.0 : sC[ixl];
        for (int s = NS - 1; s > seg; --s) u = sA[s * TX + ixl] * u + sB[s * TX + ixl];
#pragma unroll
        for (int i = SEG - 1; i >= 0; --i) { u = w[i] - Lv[i + 1] * u; w[i] = u; }
        ucar = w[0];
        const double ulo = zin * dinv_s - Lv[0] * w[0];         // u at the lower face of this segment
#pragma unroll
        for (int i = 0; i < SEG; ++i) {                          // values first, branch-free, then the stores (see schur_s_tile)
            const double lo = i == 0 ? ulo : w[i > 0 ? i - 1 : 0];
            yo[i] = yo[i] + Ta * (w[i] - lo);
        }
#pragma unroll
        for (int i = 0; i < SEG; ++i)
            if (FULL || (valid && c0 + i < n)) *reinterpret_cast<double *>(reinterpret_cast<char *>(y) + (o0 + (unsigned)i * slb)) = yo[i];
    }
    if (need_dot) {
        const double s = block_sum(Ta * dot, sred);
        if (threadIdx.x == 0) partials[(long)by * gridDim.x + bx] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// Fused-direction Schur apply for small and medium meshes (undivided, lean CG).  Below a few million cells a CG iteration is
// a chain of short dependent kernels and their number, not the bytes, sets the pace.  The x, y and z passes of one apply
// depend on each other only through the read-modify-write of y, so here they run side by side in ONE launch, each direction
// into an output vector of its own (qx = C p + X p, qy = Y p, qz = Z p; k_cg_rupdate3 forms (qx + qy) + qz, the same bits as the
// three accumulating passes).  The deferred x_sol += alpha p, p = r + beta p rides in the x blocks, which write the new p into
// the other buffer of a pair; the y / z blocks form r + beta p from the old one on the fly (CgFuse).  A CG iteration is then two
// dependent launches (k_apply3, k_cg_rupdate3) instead of four; every block of a launch first sums the partials of the
// launch before it (lean CG), so the scalars alpha, beta and the stop test need no launch of their own.
// Blocks [0, nbx) do the x lines (one wave-task per wave), [nbx, nbx+nby) one y tile each, the rest one z tile each.
struct Apply3 {
    int nbx, nby, nbz;                  // blocks per role
    int ntask_x, lpl_log2;              // x: wave-tasks per transverse mode
    int n[2], TX[2], NSEG[2], gx[2], gy[2]; long sl[2], ostride[2];   // y (index 0) and z (index 1) tiles
    long long *stamps;                  // diagnostic builds (-DNF_STAMPS): in-kernel cycle stamps of three blocks, else unused
};
template <int NCH, bool VEC, int NB, int SEG>                    // (streaming loads lose here at every size up to 4 Mi cells: 128^3 79 -> 91 us per CG iteration)
__global__ __launch_bounds__(512) void k_apply3(ModeArgs max0, ModeArgs may0, ModeArgs maz0, ModeTab mtx, ModeTab mty, ModeTab mtz, Geom G,
                                                const double *__restrict__ Lx, const double *__restrict__ DRx, const double *__restrict__ D0x,
                                                const double *__restrict__ Ly, const double *__restrict__ DRy, const double *__restrict__ D0y,
                                                const double *__restrict__ Lz, const double *__restrict__ DRz, const double *__restrict__ D0z,
                                                int nx, int ny, long nlines_x, Apply3 A, double *__restrict__ partials,
                                                const CgScalars *__restrict__ cg, CgFuse fz, CgLean lean)
{
    extern __shared__ double sm[];
    double *sred = sm + 4 * (int)blockDim.x + 320;               // behind the largest tile's scan arrays (<= 4 TX (NSEG+1) + TX doubles, TX NSEG <= blockDim, TX <= 64)
    long long *stamp = nullptr;
#ifdef NF_STAMPS
    if (A.stamps && threadIdx.x == 0) {
        if (blockIdx.x == 0) stamp = A.stamps; else if (blockIdx.x == (unsigned)A.nbx) stamp = A.stamps + 16; else if (blockIdx.x == (unsigned)(A.nbx + A.nby)) stamp = A.stamps + 32;
    }
    long long st_r0 = 0, st_0 = 0, st_1 = 0;
    if (stamp) { st_r0 = (long long)__builtin_amdgcn_s_memrealtime(); st_0 = (long long)__builtin_readcyclecounter(); }
#endif
    // scalars of the previous iteration: requested here, consumed inside `mid` -- the pass's own loads go out in between, so the
    // block pays ONE memory round trip for flags, scalars, partial sums and tile data instead of four in a row
    const int done0 = cg->done;
    const bool fuse = !lean.first;
    const double alpha0 = fuse ? cg->alpha : 0.0;
    LeanPre pre = { 0.0, 0.0, 0, 0 };
    if (fuse) pre = lean_preload(lean);
    bool stopped = false;
    auto mid = [&](double &fa, double &fb) -> bool {
        (void)fa;
        if (done0) { stopped = true; return true; }
#ifdef NF_STAMPS
        if (stamp) st_1 = (long long)__builtin_readcyclecounter();
#endif
        if (fuse) stopped = lean_rr_step(lean, pre, blockIdx.x == 0 && threadIdx.x == 0, sred, &fb);   // FIN_RR of the previous iteration: beta, stop tests
        NF_STAMP(stamp, 2);
        return stopped;
    };
    const unsigned b = blockIdx.x;
    double dot = 0.0;
    if (b < (unsigned)A.nbx) {
        const int nw = blockDim.x >> 6;
        const long gt = (long)b * nw + (threadIdx.x >> 6);      // global wave-task: mode-major
        const int mode = (int)(gt / A.ntask_x);
        const bool active = mode < mtx.n;
        const ModeArgs ma = select_mode(max0, mtx, active ? mode : 0, NB + 1);
        dot = schur_x_task<2, NCH, VEC, NB>(ma, G, Lx, DRx, D0x, nx, ny, nlines_x, A.lpl_log2, 1, gt % A.ntask_x, threadIdx.x & 63, active,
                                            fuse, alpha0, 0.0, fz, mid);
    } else {
        const int r = b < (unsigned)(A.nbx + A.nby) ? 0 : 1;
        const unsigned t = b - A.nbx - (r ? A.nby : 0);
        const unsigned bx = t % A.gx[r], by = (t / A.gx[r]) % A.gy[r], bz = t / (A.gx[r] * A.gy[r]);
        SlabArgs sa; sa.if_lo = sa.if_hi = sa.mode = sa.xcd = sa.wsmin = sa.fold = sa.noacc = 0; sa.yadd = nullptr; sa.alo = sa.ahi = sa.ulo = sa.uhi = sa.rlo = sa.rhi = sa.sinv_lo = sa.sinv_hi = nullptr; sa.clo = sa.chi = sa.jz = sa.jzb = nullptr; sa.nfa = 1; sa.ni = 0;
        if (r == 0) {
            const ModeArgs ma = select_mode(may0, mty, bz, NB + 1);
            dot = schur_s_tile<SEG, 1, false, NB>(ma, G, Ly, DRy, D0y, A.n[0], A.sl[0], A.ostride[0], nx, A.TX[0], A.NSEG[0], bx, by, bz, A.gy[0],
                                                  (int)threadIdx.x, true, sm, sa, fz, false, fuse, alpha0, 0.0, false, stamp, mid);
        } else {
            const ModeArgs ma = select_mode(maz0, mtz, bz, NB + 1);
            dot = schur_s_tile<SEG, 2, false, NB>(ma, G, Lz, DRz, D0z, A.n[1], A.sl[1], A.ostride[1], nx, A.TX[1], A.NSEG[1], bx, by, bz, A.gy[1],
                                                  (int)threadIdx.x, true, sm, sa, fz, false, fuse, alpha0, 0.0, false, stamp, mid);
        }
    }
    if (stopped) return;
    NF_STAMP(stamp, 8);
    const double sdot = block_sum(dot, sred);
    if (threadIdx.x == 0) partials[b] = sdot;
    NF_STAMP(stamp, 9);
#ifdef NF_STAMPS
    if (stamp) { stamp[13] = (long long)__builtin_amdgcn_s_memrealtime(); stamp[12] = st_r0; stamp[0] = st_0; stamp[1] = st_1; }
#endif
}
// r -= alpha ((qx + qy) + qz), |r|^2 partials; consumes the x.y partials of k_apply3 (FIN_PAP).  qy / qz may be null (1D / 2D).
template <bool MASK>
__global__ __launch_bounds__(256) void k_cg_rupdate3(double *__restrict__ r, const double *__restrict__ qx, const double *__restrict__ qy,
                                                     const double *__restrict__ qz, long n, const CgScalars *__restrict__ cg,
                                                     double *__restrict__ partials, CgLean lean, VoidMask vm)
{
    __shared__ double sred[4];
    // flags, |r|^2 of this iteration and the first trip's vector entries are requested before the reduction of the p.q partials
    // (one memory round trip instead of three in a row; on the latency-bound meshes this kernel is one trip long)
    const int done0 = cg->done;
    const double rr_cur = lean.st->rr2[lean.par];
    const long i0 = blockIdx.x * 256L + threadIdx.x;
    double r0 = 0.0, q0 = 0.0;
    bool v0 = false;
    if (i0 < n) { r0 = r[i0]; q0 = qx[i0]; if (qy) q0 += qy[i0]; if (qz) q0 += qz[i0]; if constexpr (MASK) v0 = void_entry(vm, i0, n); }
    if (done0) return;
    const double pq = strided_total(lean.partials, lean.count, sred);
    const bool brk = fabs(pq) < 1e-30;
    const double alpha = brk ? 0.0 : rr_cur / pq;
    if (blockIdx.x == 0 && threadIdx.x == 0) { lean.st->pAp = pq; lean.st->pend = 0; if (brk) lean.st->done = 1; else lean.st->alpha = alpha; }
    if (brk) return;
    double s = 0.0;
    if (i0 < n) { double rn = r0 - alpha * q0; if (MASK && v0) rn = 0.0; r[i0] = rn; s += rn * rn; }
    for (long i = i0 + gridDim.x * 256L; i < n; i += gridDim.x * 256L) {
        double q = qx[i];
        if (qy) q += qy[i];
        if (qz) q += qz[i];
        double rn = r[i] - alpha * q;
        if constexpr (MASK) if (void_entry(vm, i, n)) rn = 0.0;
        r[i] = rn; s += rn * rn;
    }
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------
// A whole CG solve (src/solvers.cpp:577-636) of a mid-size undivided mesh (any order) in ONE launch, on the workgroups of ONE XCD.
// Between the one-workgroup resident kernel (a few thousand unknowns) and the meshes that fill the chip, a CG iteration is two
// dependent launches (k_apply3, k_cg_rupdate3) whose cost is the launch boundary itself: 7.2 + 4.3 us of kernels that mostly wait for
// their first loads (L2 was written back at the boundary) plus 3.7 us of gap, on IAEA-3D 38x38x19.  The two reductions of an
// iteration need two grid-wide synchronisations; inside one launch those are barriers on a counter, and a barrier among the 32 compute
// units that share one L2 costs 0.93 us (profiles/tools/xcd_barrier.hip, profiles/r03_w_xcd_barrier.txt: two barriers + a 4 KB
// hand-off per workgroup 1.86 us with L1-bypassing loads, 3.7 us with an agent acquire per barrier, 8.9 us with release + acquire).
//   * 8 W workgroups are launched; a workgroup reads its XCD from HW_REG_XCC_ID, registers, and leaves unless it sits on XCD `xcc`.
//     Placement is observed, not assumed: the P workgroups that registered share the work, whatever P is (round-robin dispatch
//     gives W).  All participants share one L2, so a store that has been acknowledged (s_waitcnt vmcnt(0)) is visible to a load
//     that bypasses the reader's L1 (non-temporal / sc1 loads: the tile functions' streaming flavour) -- no L2 write-back
//     (buffer_wbl2), no L1 invalidate.  Uniform reads of exchanged words are explicit sc1 loads (a plain one may become a scalar
//     load through the scalar cache, which nothing here invalidates).
//   * every spin is bounded.  Workgroups that do not assemble (P = 0, P > 64, a start that times out: the XCD is busy with somebody
//     else's kernel) end the launch with CgScalars::err = 3 before a single vector has been touched and the host runs the solve
//     through the launch path; a barrier that times out in the middle of a solve (err = 4) is an error.
//   * every workgroup derives alpha, beta and the stop tests itself from the same partial sums in the same order: control flow is
//     uniform across workgroups without flags, and no scalar lives in memory during the solve.
// Phase A of an iteration = what k_apply3 does (q_x = C p + X p with the deferred x_sol += alpha p, p' = r + beta p written to the
// other buffer of the pair; q_y = Y p, q_z = Z p from p formed on the fly; p.q partials), phase B = k_cg_rupdate3.  Inside a
// 768-thread workgroup (XCD_THREADS) the three roles run side by side on different wavefronts (x: one wave-task per wave; y / z: sub-tiles of
// TX NSEG threads packed into the role's waves; the x waves keep the two barriers of a tile company).
// Partial sums: one per workgroup, added by wave_sum's fixed tree over the workgroups -- not the order of the launch path, so the iterates differ from it in
// the last bits (like the resident kernel's do); every run gives the same bits.
struct ResidentOut { double keff; int n_outer, status, cg_total, pad; };   // status 0 ok, 2 diverged (non-finite k or dphi); k_keff_xcd: 3 not assembled, 4 barrier timeout
struct XcdState { unsigned arrived, nreg, count, timeout, go; };   // go: 0 undecided, 1 start (every workgroup has registered), 2 do not start
struct XcdArgs {
    ModeArgs ma[3]; Geom G;
    const double *L[3], *DR[3], *D0[3];
    int nx, ny, dim; long nlines_x, N;
    int ntask_x, lpl_log2;
    int n[2], TX[2], NSEG[2], gx[2], gy[2]; long sl[2], ostride[2];   // y (0) and z (1) tiles
    ModeTab mt[3]; int nmodes;                                        // transverse modes of every direction (orders with bubble moments; one mode for P0)
    double *pA, *pB, *r, *xsol; const double *q[3];
    CgScalars *cg; double *part;                                      // part: 4 rotating slots of 64 partials (xcd_total), then p.q | |r|^2 partials of the CG, then diagnostics: 512 doubles
    XcdState *st; HostPub *hp; unsigned long long seq; int xcc;
};
__device__ __forceinline__ unsigned xld(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// bounded by wall time (s_memrealtime: 100 MHz, independent of the shader clock), not by an iteration count: 0.5 s -- only a lost
// participant gets there; a workgroup that was merely preempted for a few milliseconds does not fail the solve
constexpr unsigned long long XCD_SPIN_TICKS = 50000000ull;
__device__ __forceinline__ bool xcd_spin(const unsigned *p, unsigned target, unsigned *timeout)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0;; ++i) {
        if (xld(p) >= target) return true;
        if ((i & 1023) == 1023) {
            if (xld(timeout)) return false;
            if (__builtin_amdgcn_s_memrealtime() - t0 > XCD_SPIN_TICKS) break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    __hip_atomic_store(timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
}
// all threads; every wave's stores have been acknowledged by L2 before thread 0 arrives
__device__ __forceinline__ bool xcd_barrier(XcdState *st, unsigned target, int *s_ok)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(&st->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_ok = xcd_spin(&st->count, target, &st->timeout) ? 1 : 0;
    }
    __syncthreads();
    return *s_ok != 0;
}
constexpr int XCD_THREADS = 768;                                 // 12 wavefronts = 3 per SIMD: 170 VGPRs (at 1024 threads the 128-VGPR budget spilled into the loop: a reload from scratch is a trip to L2 there)
// what a workgroup knows once the participants have assembled: its index, their number, and how its wavefronts split among the roles
struct XcdCtx {
    int widx, P; bool ok;
    int R, wx, dx, role;                                          // rounds of phase A; x role: wavefronts per round, wave-tasks of this workgroup
    int sT, sC, sPer, sNt, sTX, sNSEG, sGx, sGy, sN, sSlot, sLtid; long sSl, sOst; bool isz; double *sSm;   // tile waves: their direction's parameters
    unsigned nbar; int nred;                                      // barriers passed; reductions made (partial slots rotate)
};
// registration: returns false for a workgroup that leaves (not on the chosen XCD).  *none: this workgroup was the last of the grid to
// start and nobody registered -- it must tell the host.
__device__ __forceinline__ bool xcd_assemble(XcdState *st, int xcc, int *s_i, XcdCtx &C, bool *none)
{
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    const bool part = (int)(id & 0xf) == xcc;
    *none = false;
    // The decision to start is ONE word that every participant reads (with a bounded spin per workgroup, one could time out
    // while another had just seen everybody arrive, and the two disagreed): the last workgroup of the grid to arrive -- every registration
    // is in by then -- writes go = 1 (or 2: nobody or too many registered); a participant whose wait expires tries to write 2; whoever
    // writes first decides for all.
    if (threadIdx.x == 0) {
        s_i[0] = part ? (int)__hip_atomic_fetch_add(&st->nreg, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
        const unsigned before = __hip_atomic_fetch_add(&st->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1 == gridDim.x) {
            const unsigned n = xld(&st->nreg);
            *none = n == 0;
            unsigned expect = 0u;
            (void)__hip_atomic_compare_exchange_strong(&st->go, &expect, (n > 0 && n <= 64) ? 1u : 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!part) return false;
    if (threadIdx.x == 0) {
        if (!xcd_spin(&st->go, 1u, &st->timeout)) { unsigned expect = 0u; (void)__hip_atomic_compare_exchange_strong(&st->go, &expect, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        s_i[2] = xld(&st->go) == 1u ? 1 : 0; s_i[1] = (int)xld(&st->nreg);
    }
    __syncthreads();
    C.widx = s_i[0]; C.P = s_i[1]; C.ok = s_i[2] != 0 && C.P <= 64;
    C.nbar = 0; C.nred = 0;
    return true;
}
__device__ __forceinline__ void xcd_plan(const XcdArgs &A, XcdCtx &C, int tid, int wave, double *sm)
{
    const int P = C.P, dim = A.dim;
    const int Ty = A.TX[0] * A.NSEG[0], Tz = A.TX[1] * A.NSEG[1];
    const int nty = dim >= 2 ? A.gx[0] * A.gy[0] * A.nmodes : 0, ntz = dim == 3 ? A.gx[1] * A.gy[1] * A.nmodes : 0;
    const int dx = (A.ntask_x * A.nmodes + P - 1) / P, ty = (nty + P - 1) / P, tz = (ntz + P - 1) / P;
    int R = 1, wx = 0, wy = 0, wz = 0, cy = 0, cz = 0;
    for (;; ++R) {
        wx = (dx + R - 1) / R; cy = (ty + R - 1) / R; cz = (tz + R - 1) / R;
        wy = (cy * Ty + 63) >> 6; wz = (cz * Tz + 63) >> 6;
        if (wx + wy + wz <= XCD_THREADS / 64 || R >= 4096) break;
    }
    if (wx + wy + wz > XCD_THREADS / 64) C.ok = false;
    C.R = R; C.wx = wx; C.dx = dx;
    C.role = wave < wx ? 0 : wave < wx + wy ? 1 : wave < wx + wy + wz ? 2 : 3;
    // y and z tiles run the same code (one unknown per cell: the direction is nothing but strides): a tile wave picks its direction's parameters once
    const bool isz = C.role == 2;
    C.isz = isz;
    C.sT = isz ? Tz : Ty; C.sC = isz ? cz : cy; C.sPer = isz ? tz : ty; C.sNt = isz ? ntz : nty;
    C.sTX = isz ? A.TX[1] : A.TX[0]; C.sNSEG = isz ? A.NSEG[1] : A.NSEG[0]; C.sGx = isz ? A.gx[1] : A.gx[0]; C.sGy = isz ? A.gy[1] : A.gy[0]; C.sN = isz ? A.n[1] : A.n[0];
    C.sSl = isz ? A.sl[1] : A.sl[0]; C.sOst = isz ? A.ostride[1] : A.ostride[0];
    const int sLt = tid - (isz ? wx + wy : wx) * 64;
    C.sSlot = sLt / C.sT; C.sLtid = sLt - C.sSlot * C.sT;
    C.sSm = sm + (isz ? cy * (4 * Ty + A.TX[0]) : 0) + ((C.sSlot >= 0 && C.sSlot < C.sC) ? C.sSlot : 0) * (4 * C.sT + C.sTX);
}
// grid-wide sum, the same bits in every thread of every participant: one partial per workgroup (block_sum), barrier, lane i fetches
// workgroup i's partial with one L1-bypassing load (P dependent loads would be P trips to L2), then wave_sum's fixed tree.  The partial
// slots rotate (four of them), so a slot is rewritten three barriers after its readers have moved on.  NV values share one barrier.
template <int NV>
__device__ __forceinline__ bool xcd_total(double (&v)[NV], double *part, XcdState *st, XcdCtx &C, double *sred, int *s_ok)
{
    const int tid = threadIdx.x, lane = tid & 63;
    double *slot[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        slot[k] = part + 64 * (C.nred++ & 3);
        const double sd = block_sum(v[k], sred);
        if (tid == 0) slot[k][C.widx] = sd;
        if (k + 1 < NV) __syncthreads();
    }
    if (!xcd_barrier(st, (unsigned)C.P * ++C.nbar, s_ok)) return false;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(lane < C.P ? __builtin_nontemporal_load(slot[k] + lane) : 0.0);
    return true;
}
// The CG solve of one group (src/solvers.cpp:577-636) by the assembled workgroups: x_sol = 0, r = p = rhs in pA and |rhs|^2 = rr are
// in place.  offN / offP / offL*: this group's offsets into the factor arrays (cells), the C diagonal (unknowns) and the first pivots (lines).
// err: 0, 1 (non-finite sum), 4 (a barrier timed out).  On return x_sol holds the solution (the deferred last update applied).
// NB > 0 (bubble moments): the wave-tasks and tiles of all transverse modes are numbered mode-major (ModeTab), y and z tiles run their own
// instantiations (the bubbles' geometry factor depends on the direction) with SEG = 4 cells per thread.
template <int NCH, bool VEC, int NB, int SEG>
__device__ __forceinline__ void xcd_cg(const XcdArgs &A, XcdCtx &C, long offN, long offP, long offL0, long offL1, long offL2, double *xsol,
                                       double &rr, double tol_sq, int maxit, int &its, int &err, double *sred, int *s_ok, long long *xs)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dim = A.dim; const long N = A.N; const int P = C.P, widx = C.widx;
    SlabArgs sa0; sa0.if_lo = sa0.if_hi = sa0.mode = sa0.xcd = sa0.wsmin = sa0.fold = sa0.noacc = 0; sa0.yadd = nullptr; sa0.alo = sa0.ahi = sa0.ulo = sa0.uhi = sa0.rlo = sa0.rhi = sa0.sinv_lo = sa0.sinv_hi = nullptr; sa0.clo = sa0.chi = sa0.jz = sa0.jzb = nullptr; sa0.nfa = 1; sa0.ni = 0;
    const double *const sL = (C.isz ? A.L[2] : A.L[1]) + offN, *const sDR = (C.isz ? A.DR[2] : A.DR[1]) + offN, *const sD0 = C.isz ? A.D0[2] + offL2 : A.D0[1] + offL1;
    ModeArgs ms = A.ma[0]; ms.Ta = C.isz ? A.ma[2].Ta : A.ma[1].Ta; ms.y[0] = C.isz ? A.ma[2].y[0] : A.ma[1].y[0];
    ModeArgs mx = A.ma[0], my = A.ma[1], mz = A.ma[2];
#pragma unroll
    for (int q = 0; q <= NB; ++q) mx.Cd[q] = A.ma[0].Cd[q] + offP;
    mx.D = A.ma[0].D + offN; my.D = A.ma[1].D + offN; mz.D = A.ma[2].D + offN;
    double alpha = 0.0, beta = 0.0, rr_new = rr;
    int pend = 0;
    double *const ppq = A.part + 256, *const prr = A.part + 320;
#ifdef NF_XSTAMPS
    long long xt = (long long)__builtin_amdgcn_s_memrealtime();
#define NF_XS(k) do { const long long t_ = (long long)__builtin_amdgcn_s_memrealtime(); xs[k] += t_ - xt; xt = t_; } while (0)
#else
    (void)xs;
#define NF_XS(k) do { } while (0)
#endif
    its = 0; err = 0;
    if (maxit > 0)
        for (;;) {
            const bool fuse = its > 0;
            double *const pin = (its == 0 || (its & 1)) ? A.pA : A.pB, *const pout = pin == A.pA ? A.pB : A.pA;
            const CgFuse fz = { pin, A.r, xsol, pout };
            // ---- phase A: q_d = S_d p for every direction, p.q
            double dot = 0.0;
            for (int ro = 0; ro < C.R; ++ro) {
                if (C.role == 1 || C.role == 2) {
                    const int k = ro * C.sC + C.sSlot, t = widx * C.sPer + k;
                    const bool act = C.sSlot < C.sC && k < C.sPer && t < C.sNt;
                    const unsigned tt = act ? t : 0;
                    if (NB == 0) {
                        ms.x[0] = pin;
                        dot += schur_s_tile<8, 1, false, 0, SV_NT, NoMid, true>(ms, A.G, sL, sDR, sD0, C.sN, C.sSl, C.sOst, A.nx, C.sTX, C.sNSEG, tt % C.sGx, tt / C.sGx, 0, C.sGy,
                                                                                              C.sLtid, act, C.sSm, sa0, fz, false, fuse, alpha, beta, false);
                    } else {
                        const unsigned per = (unsigned)(C.sGx * C.sGy), bz = tt / per, rem = tt - bz * per;
                        if (C.role == 1) {
                            ModeArgs m = my;
#pragma unroll
                            for (int q = 0; q <= NB; ++q) { m.x[q] = pin + (A.ma[1].x[q] - A.pA); m.Cd[q] = nullptr; }
                            m = select_mode(m, A.mt[1], bz, NB + 1);
                            dot += schur_s_tile<SEG, 1, false, NB, SV_NT, NoMid, true>(m, A.G, sL, sDR, sD0, C.sN, C.sSl, C.sOst, A.nx, C.sTX, C.sNSEG, rem % C.sGx, rem / C.sGx, bz, C.sGy,
                                                                                                    C.sLtid, act, C.sSm, sa0, fz, false, fuse, alpha, beta, false);
                        } else {
                            ModeArgs m = mz;
#pragma unroll
                            for (int q = 0; q <= NB; ++q) { m.x[q] = pin + (A.ma[2].x[q] - A.pA); m.Cd[q] = nullptr; }
                            m = select_mode(m, A.mt[2], bz, NB + 1);
                            dot += schur_s_tile<SEG, 2, false, NB, SV_NT, NoMid, true>(m, A.G, sL, sDR, sD0, C.sN, C.sSl, C.sOst, A.nx, C.sTX, C.sNSEG, rem % C.sGx, rem / C.sGx, bz, C.sGy,
                                                                                                    C.sLtid, act, C.sSm, sa0, fz, false, fuse, alpha, beta, false);
                        }
                    }
                } else {
                    const int k = ro * C.wx + wave; const long gt = (long)widx * C.dx + k;
                    const bool act = C.role == 0 && k < C.dx && gt < (long)A.ntask_x * A.nmodes;
                    const int mode = act ? (int)(gt / A.ntask_x) : 0;
                    ModeArgs m = mx;
#pragma unroll
                    for (int q = 0; q <= NB; ++q) m.x[q] = pin + (A.ma[0].x[q] - A.pA);
                    if (NB > 0) m = select_mode(m, A.mt[0], mode, NB + 1);
                    dot += schur_x_task<2, NCH, VEC, NB, NoMid, true, true>(m, A.G, A.L[0] + offN, A.DR[0] + offN, A.D0[0] + offL0, A.nx, A.ny, A.nlines_x, A.lpl_log2, 1,
                                                                           act ? gt - (long)mode * A.ntask_x : 0, lane, act, fuse, alpha, beta, fz);
                    __syncthreads(); __syncthreads();           // the two barriers inside a y / z tile
                }
                __syncthreads();                                 // the tiles' scan arrays are reused by the next round
            }
            NF_XS(0);
            { const double sd = block_sum(dot, sred); if (tid == 0) ppq[widx] = sd; }
            NF_XS(1);
            if (!xcd_barrier(A.st, (unsigned)P * ++C.nbar, s_ok)) { err = 4; break; }
            NF_XS(2);
            const double pq = wave_sum(lane < P ? __builtin_nontemporal_load(ppq + lane) : 0.0);     // src/solvers.cpp:602-606
            NF_XS(3);
            pend = 0;
            if ((pq - pq) != 0.0) { err = 1; rr = pq; break; }
            if (fabs(pq) < 1e-30) break;
            alpha = rr / pq;
            // ---- phase B: r -= alpha ((q_x + q_y) + q_z), |r|^2
            // (all loads of an element go out before the first use: a load inside a predicated region is waited for there, one trip
            // to L2 per operand instead of one per element; for dim < 3 the missing directions point at q_x and are not added)
            double s = 0.0;
            for (long i = (long)widx * XCD_THREADS + tid; i < N; i += (long)P * XCD_THREADS) {
                const double q0 = __builtin_nontemporal_load(A.q[0] + i), q1 = __builtin_nontemporal_load(A.q[1] + i), q2 = __builtin_nontemporal_load(A.q[2] + i);
                const double r0 = __builtin_nontemporal_load(A.r + i);
                double q = q0;
                if (dim >= 2) q += q1;
                if (dim == 3) q += q2;
                const double rn = r0 - alpha * q;
                A.r[i] = rn; s += rn * rn;
            }
            { const double sd = block_sum(s, sred); if (tid == 0) prr[widx] = sd; }
            NF_XS(4);
            if (!xcd_barrier(A.st, (unsigned)P * ++C.nbar, s_ok)) { err = 4; break; }
            NF_XS(5);
            rr_new = wave_sum(lane < P ? __builtin_nontemporal_load(prr + lane) : 0.0);               // :613-631
            if ((rr_new - rr_new) != 0.0) { err = 1; rr = rr_new; break; }
            ++its; pend = 1;
            NF_XS(6);
            if (rr_new < tol_sq) { rr = rr_new; break; }
            beta = rr_new / rr; rr = rr_new;
            if (its >= maxit) break;
        }
    // ---- the last iteration's x_sol += alpha p (:609); its direction: see the buffer pair in cg_solve
    if (pend && !err) {
        const double *plast = (its >= 2 && ((its - 1) & 1)) ? A.pB : A.pA;
        for (long i = (long)widx * XCD_THREADS + tid; i < N; i += (long)P * XCD_THREADS)
            xsol[i] = fma(alpha, __builtin_nontemporal_load(plast + i), __builtin_nontemporal_load(xsol + i));
    }
}
template <int NCH, bool VEC, int NB = 0, int SEG = 8>
__global__ __launch_bounds__(XCD_THREADS) void k_cg_xcd(XcdArgs A)
{
    extern __shared__ double sm[];
    __shared__ int s_i[4];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *const sred = sm + 5 * 1024 + 64;
    XcdCtx C; bool none;
    const bool part = xcd_assemble(A.st, A.xcc, s_i, C, &none);
    if (none) {                                                   // nobody sits on the chosen XCD: say so
        A.cg->err = 3; A.cg->done = 1;
        if (A.hp) { A.hp->cg = *A.cg; __threadfence_system(); __hip_atomic_store(&A.hp->seq, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
    }
    if (!part) return;
    xcd_plan(A, C, tid, wave, sm);
    // ---- scalars as k_finalize(FIN_RHS) left them (a launch earlier)
    double rr = A.cg->rr;
    const double tol_sq = A.cg->tol_sq; const int maxit = A.cg->maxit;
    int its = 0, err = C.ok ? 0 : 3;
    long long xs[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (C.ok && !A.cg->done) xcd_cg<NCH, VEC, NB, SEG>(A, C, 0, 0, 0, 0, 0, A.xsol, rr, tol_sq, maxit, its, err, sred, &s_i[3], xs);
#ifdef NF_XSTAMPS
    if (C.widx == 0 && tid == 0) { for (int k = 0; k < 7; ++k) A.part[384 + k] += (double)xs[k]; A.part[391] += its; A.part[392] += 1; A.part[393] = C.P; A.part[394] = C.R; A.part[395] = C.wx; }
#endif
    if (C.widx == 0 && tid == 0) {
        CgScalars *cg = A.cg;
        if (!cg->done || err) { cg->rr = rr; cg->rr_new = rr; cg->its = its; cg->pend = 0; cg->done = 1; cg->err = err; }
        if (A.hp) { A.hp->cg = *cg; __threadfence_system(); __hip_atomic_store(&A.hp->seq, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
    }
}

// The whole SolveKeff (src/NeutFEM.cpp:1627-1815: fission source, Gauss-Seidel group sweep with CG, k update, normalisation, Chebyshev,
// stop tests, history) of the same meshes in ONE launch on the workgroups of one XCD: what k_resident_keff does in one workgroup for
// meshes that fit its LDS, with grid barriers in the place of workgroup barriers.  Beside the CG iterations themselves this removes
// what surrounds them on the host-driven path: per group solve five stream operations and a host check, per outer iteration four
// launches and a host check (IAEA-3D 38x38x19: ~6 ms of 22).  Elementwise loops are grid-strided; every vector is read with
// L1-bypassing loads, and a barrier separates every phase that writes a vector from the phases that read it under another ownership.
// Every workgroup carries the scalars (k, Chebyshev state, stop tests) itself, from the same sums: uniform control flow, no flags.
struct XcdOuter {
    int ng; long NP, N;
    const double *Mf, *Chi; const double *const *Ms;
    double *phi, *raw, *p0, *p1, *tf;
    long nl[3];
    double keff0, tol_keff, tol_flux, cg_tol; int cg_max, max_outer;
    ChebTable cheb;
    double *hist; int *hist_cg; ResidentOut *out;                // status 3: the workgroups did not assemble (nothing touched), 4: a barrier timed out
};
template <int NCH, bool VEC, int NB = 0, int SEG = 8>
__global__ __launch_bounds__(XCD_THREADS) void k_keff_xcd(XcdArgs A, XcdOuter O)
{
    extern __shared__ double sm[];
    __shared__ int s_i[4];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *const sred = sm + 5 * 1024 + 64;
    XcdCtx C; bool none;
    const bool part = xcd_assemble(A.st, A.xcc, s_i, C, &none);
    if (none) { O.out->keff = O.keff0; O.out->n_outer = 0; O.out->status = 3; O.out->cg_total = 0; }
    if (!part) return;
    xcd_plan(A, C, tid, wave, sm);
    if (!C.ok) { if (C.widx == 0 && tid == 0) { O.out->keff = O.keff0; O.out->n_outer = 0; O.out->status = 3; O.out->cg_total = 0; } return; }
    const int ng = O.ng; const long NP = O.NP, N = O.N, NT = NP * ng;
    const long g0 = (long)C.widx * XCD_THREADS + tid, gs = (long)C.P * XCD_THREADS;
    double keff = O.keff0;
    int cheb_it = 0, n_outer = 0, status = 0, cg_total = 0;
    double *pa = O.p0, *pb = O.p1;
    long long xs[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int it = 0; it < O.max_outer && !status; ++it) {
        // total_fiss and prod_old (:1700-1707)
        double v1[1] = { 0.0 };
        for (long i = g0; i < NP; i += gs) {
            double v = 0.0;
            for (int g = 0; g < ng; ++g) v += O.Mf[g * NP + i] * __builtin_nontemporal_load(O.phi + g * NP + i);
            O.tf[i] = v; v1[0] += v;
        }
        if (!xcd_total<1>(v1, A.part, A.st, C, sred, &s_i[3])) { status = 4; break; }
        const double prod_old = v1[0];
        const double inv_k = 1.0 / keff;
        for (int g = 0; g < ng && !status; ++g) {
            double *const graw = O.raw + (long)g * NP;
            // rhs = chi_g tf / k + scatter (Gauss-Seidel) (:1716-1726); CG start x = 0, r = p = rhs (src/solvers.cpp:583-592)
            v1[0] = 0.0;
            for (long i = g0; i < NP; i += gs) {
                double v;
                if (NB == 0) v = inv_k * (O.Chi[g * N + i] * __builtin_nontemporal_load(O.tf + i));
                else { const double cv = O.Chi[g * N + i % N] * inv_k; v = fabs(cv) < 1e-14 ? 0.0 : cv * __builtin_nontemporal_load(O.tf + i); }   // BuildFissionRHS, P >= 1 (:1539-1561)
                for (int gp = 0; gp < ng; ++gp) {
                    const double *M = O.Ms[g * ng + gp];
                    if (gp == g || !M) continue;
                    v += M[i] * __builtin_nontemporal_load((gp < g ? O.raw : O.phi) + gp * NP + i);
                }
                graw[i] = 0.0; A.r[i] = v; A.pA[i] = v; v1[0] += v * v;
            }
            if (!xcd_total<1>(v1, A.part, A.st, C, sred, &s_i[3])) { status = 4; break; }
            double rr = v1[0];
            const double rhs_norm = sqrt(rr), tol_sq = O.cg_tol * O.cg_tol * rhs_norm * rhs_norm;
            int its = 0, err = 0;
            xcd_cg<NCH, VEC, NB, SEG>(A, C, g * N, g * NP, g * O.nl[0], g * O.nl[1], g * O.nl[2], graw, rr, tol_sq, O.cg_max, its, err, sred, &s_i[3], xs);
            if (err == 4) { status = 4; break; }
            if (err == 1) status = 2;                             // a non-finite sum: the outer iteration below reports the divergence
            if (tid == 0 && C.widx == 0) O.hist_cg[it * ng + g] = its;
            cg_total += its;
            if (!xcd_barrier(A.st, (unsigned)C.P * ++C.nbar, &s_i[3])) { status = 4; break; }   // this group's solution is complete before anybody reads it
        }
        if (status == 4) break;
        // prod_new, norms (:1766-1779)
        double v3[3] = { 0.0, 0.0, 0.0 };
        for (long i = g0; i < NT; i += gs) { const double v = __builtin_nontemporal_load(O.raw + i), d = v - __builtin_nontemporal_load(O.phi + i); v3[0] += O.Mf[i] * v; v3[1] += v * v; v3[2] += d * d; }
        if (!xcd_total<3>(v3, A.part, A.st, C, sred, &s_i[3])) { status = 4; break; }
        const OuterStep os = outer_step(keff, it, prod_old, v3[0], v3[1], v3[2]);
        keff = os.keff;
        if (tid == 0 && C.widx == 0) { O.hist[it] = keff; O.hist[O.max_outer + it] = os.dk; O.hist[2 * O.max_outer + it] = os.dphi; }
        n_outer = it + 1;
        if (!os.finite) { status = 2; break; }
        status = 0;
        // normalise + Chebyshev (:1780-1788, src/solvers.cpp:720-756)
        const ChebStep cs = cheb_next(cheb_it, O.cheb, it >= 2);
        for (long i = g0; i < NT; i += gs) O.phi[i] = cheb_update(__builtin_nontemporal_load(O.raw + i), os.do_norm, os.norm, cs, pa, pb, i);
        if (cs.mode == 3) { double *t = pa; pa = pb; pb = t; }
        if (!xcd_barrier(A.st, (unsigned)C.P * ++C.nbar, &s_i[3])) { status = 4; break; }   // the new phi before the next fission source
        if (outer_converged(os.dk, os.dphi, O.tol_keff, O.tol_flux)) break;   // :1799-1802
    }
    if (tid == 0 && C.widx == 0) { O.out->keff = keff; O.out->n_outer = n_outer; O.out->status = status; O.out->cg_total = cg_total; }
}

// ---------------------------------------------------------------------------------------------
// CG vector kernels (src/solvers.cpp:577-631).  Fixed grids, grid-stride loops.
// MASK (nf_set_void, VoidMask above): the residual is written as 0 in the void cells and stays out of |r|^2; the right-hand side counts as 0 there
template <bool MASK>
__global__ __launch_bounds__(256) void k_cg_init(const double *__restrict__ rhs, double *__restrict__ x,
                                                 double *__restrict__ r, double *__restrict__ p, long n,
                                                 double *__restrict__ partials, VoidMask vm)
{
    __shared__ double sred[4];
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        double b = rhs[i];
        if constexpr (MASK) if (void_entry(vm, i, n)) b = 0.0;
        x[i] = 0.0; r[i] = b; p[i] = b; s += b * b;
    }
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
template <bool MASK>
__global__ __launch_bounds__(256) void k_cg_update(double *__restrict__ x, double *__restrict__ r,
                                                   const double *__restrict__ p, const double *__restrict__ q, long n,
                                                   const CgScalars *__restrict__ cg, double *__restrict__ partials, VoidMask vm)
{
    __shared__ double sred[4];
    if (cg->done) return;
    const double alpha = cg->alpha;
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        x[i] = fma(alpha, p[i], x[i]);
        double rn = r[i] - alpha * q[i];
        if constexpr (MASK) if (void_entry(vm, i, n)) rn = 0.0;
        r[i] = rn; s += rn * rn;
    }
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// fused CG: r -= alpha q and |r|^2 only (x_sol and p are updated by the next x pass)
template <bool MASK>
__global__ __launch_bounds__(256) void k_cg_rupdate(double *__restrict__ r, const double *__restrict__ q, long n,
                                                    const CgScalars *__restrict__ cg, double *__restrict__ partials, CgLean lean, VoidMask vm)
{
    __shared__ double sred[4];
    if (cg->done) return;
    double alpha;
    if (lean.st) {                                              // lean CG: this kernel consumes the p.q partials (FIN_PAP)
        const double pq = lean_total(lean, sred);
        const int e = lean_err(lean, pq);
        if (e) { if (blockIdx.x == 0 && threadIdx.x == 0) { lean.st->pAp = pq; lean.st->err = e; lean.st->done = 1; } return; }
        const bool brk = fabs(pq) < 1e-30;
        alpha = brk ? 0.0 : lean.st->rr2[lean.par] / pq;
        if (blockIdx.x == 0 && threadIdx.x == 0) { lean.st->pAp = pq; lean.st->pend = 0; if (brk) lean.st->done = 1; else lean.st->alpha = alpha; }
        if (brk) return;
    } else alpha = cg->alpha;
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        double rn = r[i] - alpha * q[i];                         // (streaming loads change nothing here: 102.3 vs 102.9 us of non-pass time per iteration)
        if constexpr (MASK) if (void_entry(vm, i, n)) rn = 0.0;
        r[i] = rn; s += rn * rn;
    }
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// fused CG: the x_sol updates that the x passes of the finished solve have not applied, in order.  ring.n < 0: the one of the final
// iteration, if CgScalars::pend says so (every form but the batched one); else ring.n updates x = fma(ah[alpha[i]], p[i], x), as the host
// derived them from the final scalars (nf_ring_pending)
struct FlushRing { int n; int alpha[8]; const double *ah; const double *p[8]; };
__global__ void k_cg_flush(double *__restrict__ x, const double *__restrict__ p, long n, const CgScalars *__restrict__ cg, FlushRing ring)
{
    if (ring.n < 0) {
        if (!cg->pend) return;
        const double alpha = cg->alpha;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) x[i] = fma(alpha, p[i], x[i]);
        return;
    }
    double a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = j < ring.n ? ring.ah[ring.alpha[j] & 7] : 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        double v = x[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < ring.n) v = fma(a[j], ring.p[j][i], v);
        x[i] = v;
    }
}
__global__ __launch_bounds__(256) void k_cg_pupdate(double *__restrict__ p, const double *__restrict__ r, long n,
                                                    const CgScalars *__restrict__ cg)
{
    if (cg->done) return;
    const double beta = cg->beta;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) p[i] = fma(beta, p[i], r[i]);
}

// ---------------------------------------------------------------------------------------------
// power iteration kernels (src/NeutFEM.cpp:1694-1788)
// total_fiss = sum_g M_fiss[g] phi_g ; partial sum of entries (prod_old)        (:1700-1707)
// With w != NULL (adjoint, :1930-1936) the partial sum is sum_{e < nw} w[e] * tf[e] (DOF 0 of every cell = first N entries).
__global__ __launch_bounds__(256) void k_fission(const double *__restrict__ Mf, const double *__restrict__ phi, int ng,
                                                 long n, double *__restrict__ tf, double *__restrict__ partials,
                                                 const double *__restrict__ w, long nw)
{
    __shared__ double sred[4];
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        double v = 0.0;
        for (int g = 0; g < ng; ++g) v += Mf[g * n + i] * phi[g * n + i];
        tf[i] = v;
        if (!w) s += v; else if (i < nw) s += w[i] * v;
    }
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
struct ScatterArgs { const double *M[64]; int ng; };
// rhs = chi_g * total_fiss / k + sum_{gp != g} M_scatter[g<-gp] phi_gp  (Gauss-Seidel: gp < g from the new
// iterate, gp > g from the old one) (:1716-1726).  If sinv != NULL the diagonal solve phi = S_inv * rhs is
// fused (:607-613) and written to out, otherwise out = rhs.
// n = DOFs per group (SoA [p][e]), ncell = cells: chi is per cell; for P>=1 elements with |chi/k| < 1e-14 are skipped (:1551).
// With r0 != nullptr the CG start of src/solvers.cpp:583-592 rides along (x = 0, r = p = rhs, block partials of |rhs|^2: what k_cg_init
// does), one launch less per group solve.
// SRC (fixed-source solve, nf_solve_subcritical): the external source q (this group's n DOFs, k_source_q) is added last; inv_k is then
// the fission scale (1: fission on, 0: the no-fission phase).  SRC = false is the eigenvalue instantiation, unchanged.
template <bool SRC>
__global__ __launch_bounds__(256) void k_group_rhs(ScatterArgs sa, int g, const double *__restrict__ chi,
                                                   const double *__restrict__ tf, double inv_k,
                                                   const double *__restrict__ phi_new, const double *__restrict__ phi_old,
                                                   const double *__restrict__ sinv, double *__restrict__ out, long n, long ncell,
                                                   double *__restrict__ x0 = nullptr, double *__restrict__ r0 = nullptr, double *__restrict__ p0 = nullptr,
                                                   double *__restrict__ partials = nullptr, const double *__restrict__ q = nullptr)
{
    __shared__ double sred[4];
    double s2 = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        double v;
        if (n == ncell) v = inv_k * (chi[i] * tf[i]);
        else { const double cv = chi[i % ncell] * inv_k; v = fabs(cv) < 1e-14 ? 0.0 : cv * tf[i]; }
        for (int gp = 0; gp < sa.ng; ++gp) {
            if (gp == g || !sa.M[gp]) continue;
            const double *ph = gp < g ? phi_new : phi_old;
            v += sa.M[gp][i] * ph[gp * n + i];
        }
        if constexpr (SRC) v += q[i];
        out[i] = sinv ? sinv[i] * v : v;
        if (r0) { x0[i] = 0.0; r0[i] = v; p0[i] = v; s2 += v * v; }
    }
    if (r0) {
        s2 = block_sum(s2, sred);
        if (threadIdx.x == 0) partials[blockIdx.x] = s2;
    }
}
// partial sums of prod_new, ||phi||^2, ||phi - phi_old||^2 over all groups       (:1766-1779)
__global__ __launch_bounds__(256) void k_outer_reduce(const double *__restrict__ Mf, const double *__restrict__ phi,
                                                      const double *__restrict__ old, long ntot,
                                                      double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    double sp = 0.0, sn = 0.0, sd = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ntot; i += gridDim.x * 256L) {
        const double v = phi[i], d = v - old[i];
        sp += Mf[i] * v; sn += v * v; sd += d * d;
    }
    sp = block_sum(sp, sred); sn = block_sum(sn, sred); sd = block_sum(sd, sred);
    if (threadIdx.x == 0) { partials[blockIdx.x] = sp; partials[stride + blockIdx.x] = sn; partials[2 * stride + blockIdx.x] = sd; }
}

// ---- fixed-source (subcritical) solve, nf_solve_subcritical ------------------------------------------------------------------------
// |e| of cell e: hx hy hz (inactive axes have width 1), the measure the fission matrix uses (k_cell_coef: C-hat_00 detJ = |e|)
__device__ __forceinline__ double cell_measure(const double *__restrict__ hx, const double *__restrict__ hy, const double *__restrict__ hz,
                                               int nx, int ny, long e)
{
    const int ix = (int)(e % nx); const long r = e / nx; const int iy = (int)(r % ny); const int iz = (int)(r / ny);
    return hx[ix] * hy[iy] * hz[iz];
}
// q = the per-cell source SRC [g*N + e] as a load vector: DOF 0 of cell e gets Q_g(e) |e|, the higher moments 0.  Output over all groups,
// SoA [g*n + p*N + e] (n = DOFs per group).  No 1e-14 drop.
__global__ __launch_bounds__(256) void k_source_q(const double *__restrict__ src, double *__restrict__ q, const double *__restrict__ hx,
                                                  const double *__restrict__ hy, const double *__restrict__ hz, int nx, int ny, long N,
                                                  long n, long ntot)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ntot; i += gridDim.x * 256L) {
        const long g = i / n, j = i - g * n;
        q[i] = j < N ? src[g * N + j] * cell_measure(hx, hy, hz, nx, ny, j) : 0.0;
    }
}
// one streaming pass over all groups after the group sweep: block partials of Phi = sum |e| phi_0, P = sum Mf_0 phi_0 (DOF 0 of every
// cell: Mf_0 = nuSigf |e|), ||phi||^2 and ||phi - old||^2 into rows 0..3 of the team partials layout; old <- phi in the same sweep
__global__ __launch_bounds__(256) void k_subcrit_reduce(const double *__restrict__ Mf, const double *__restrict__ phi, double *__restrict__ old,
                                                        const double *__restrict__ hx, const double *__restrict__ hy, const double *__restrict__ hz,
                                                        int nx, int ny, long N, long n, long ntot, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    double sf = 0.0, sp = 0.0, sn = 0.0, sd = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ntot; i += gridDim.x * 256L) {
        const double v = phi[i], d = v - old[i];
        sn += v * v; sd += d * d;
        old[i] = v;
        const long j = i - (i / n) * n;
        if (j < N) { sf += cell_measure(hx, hy, hz, nx, ny, j) * v; sp += Mf[i] * v; }
    }
    sf = block_sum(sf, sred); sp = block_sum(sp, sred); sn = block_sum(sn, sred); sd = block_sum(sd, sred);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sf; partials[stride + blockIdx.x] = sp;
        partials[2 * stride + blockIdx.x] = sn; partials[3 * stride + blockIdx.x] = sd;
    }
}

// ---- space-time kinetics, nf_transient_step ---------------------------------------------------------------------------
// All streaming grid-stride kernels in the style of k_subcrit_reduce: block partials in a fixed order (rows of `stride` doubles), summed
// by k_finalize.  Vectors are SoA [g*n + p*N + e] (n = DOFs per group), per-cell arrays [g*N + e].
struct TrGroups { double v[64]; };                               // one value per group
struct TrFamilies { int n; double a[NF_PRECURSORS_MAX], b[NF_PRECURSORS_MAX]; };   // two coefficients per precursor family
// SigR of the step operator: SigR_g + 1 / (v_g dt) (shift.v[g]), all groups
__global__ __launch_bounds__(256) void k_tr_shift(const double *__restrict__ sigr, double *__restrict__ out, long N, long ntot, TrGroups shift)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ntot; i += gridDim.x * 256L) out[i] = sigr[i] + shift.v[i / N];
}
// chi~_g(e) = chi_g(e) - chi_d,g(e) a: chi_d the ng values of `chid`, or chi itself (per_cell)
__global__ __launch_bounds__(256) void k_tr_chi(const double *__restrict__ chi, double *__restrict__ out, long N, long ntot, TrGroups chid,
                                                int per_cell, double a)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ntot; i += gridDim.x * 256L) {
        const double c = chi[i];
        out[i] = c - (per_cell ? c : chid.v[i / N]) * a;
    }
}
// W_p(e) = detJ(e) C-hat_pp, the mass weight of a unit cross section (|e| at P0): k_cell_coef's values for xs = 1 without its drop
__global__ __launch_bounds__(256) void k_tr_weights(double *__restrict__ W, const double *__restrict__ hx, const double *__restrict__ hy,
                                                    const double *__restrict__ hz, int nx, int ny, long N, int dim, ChatArgs ch)
{
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        const int ix = (int)(e % nx); const long r = e / nx; const int iy = (int)(r % ny); const int iz = (int)(r / ny);
        if (ch.nloc == 1) { W[e] = hx[ix] * hy[iy] * hz[iz]; continue; }
        double detJ = hx[ix] / 2.0;
        if (dim >= 2) detJ *= hy[iy] / 2.0;
        if (dim == 3) detJ *= hz[iz] / 2.0;
        for (int p = 0; p < ch.nloc; ++p) W[(long)p * N + e] = detJ * ch.c[p];
    }
}
// step source of all groups in one pass: q_g = W phi_g ivdt_g + chi_d,g sum_i fam.a[i] c_i with fam.a[i] = lambda_i / (1 + lambda_i dt),
// ivdt_g = 1 / (v_g dt); chi_d as in k_tr_chi.  Row 0 of the partials: Q = the sum of q over the DOF-0 rows (j < N) of all groups
__global__ __launch_bounds__(256) void k_tr_source(const double *__restrict__ phi, const double *__restrict__ c, const double *__restrict__ W,
                                                   const double *__restrict__ chi, double *__restrict__ q, long N, long n, int ng,
                                                   TrGroups ivdt, TrGroups chid, int per_cell, TrFamilies fam, double *__restrict__ partials)
{
    __shared__ double sred[4];
    double sq = 0.0;
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n; j += gridDim.x * 256L) {
        double d = 0.0;
        for (int i = 0; i < fam.n; ++i) d += fam.a[i] * c[i * n + j];
        const double w = W[j]; const long e = j % N;
        for (int g = 0; g < ng; ++g) {
            const double v = w * phi[g * n + j] * ivdt.v[g] + (per_cell ? chi[g * N + e] : chid.v[g]) * d;
            q[g * n + j] = v;
            if (j < N) sq += v;
        }
    }
    sq = block_sum(sq, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = sq;
}
// U of the rebalance: the sum of the DOF-0 rows of the right-hand side the group solve is about to use (its first N entries), added to
// the partial of the groups before it (first = 1: the row starts here).  k_group_rhs itself stays as it is.
__global__ __launch_bounds__(256) void k_tr_rhs_sum(const double *__restrict__ rhs, long N, double *__restrict__ partials, int first)
{
    __shared__ double sred[4];
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < N; i += gridDim.x * 256L) s += rhs[i];
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = first ? s : partials[blockIdx.x] + s;
}
// E of the rebalance: what the DOF-0 rows of k_group_rhs<true> would hold for the NEW iterate y without q, summed over all groups -- tf as
// k_fission forms it, the emission and the scatter terms by k_group_rhs's own expressions and drop rule (a mismatch would move the fixed
// point of the iteration).  Ms: the ng*ng device pointers [g*ng + gp] (nullptr: empty block).
__global__ __launch_bounds__(256) void k_tr_emission(const double *__restrict__ Mf, const double *__restrict__ y, const double *__restrict__ chi,
                                                     const double *const *__restrict__ Ms, double inv_k, long N, long n, int ng,
                                                     double *__restrict__ partials)
{
    __shared__ double sred[4];
    double se = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < N; i += gridDim.x * 256L) {
        double tf = 0.0;
        for (int g = 0; g < ng; ++g) tf += Mf[g * n + i] * y[g * n + i];
        for (int g = 0; g < ng; ++g) {
            double v;
            if (n == N) v = inv_k * (chi[g * N + i] * tf);
            else { const double cv = chi[g * N + i] * inv_k; v = fabs(cv) < 1e-14 ? 0.0 : cv * tf; }
            for (int gp = 0; gp < ng; ++gp) {
                const double *M = Ms[g * ng + gp];
                if (gp == g || !M) continue;
                v += M[i] * y[gp * n + i];
            }
            se += v;
        }
    }
    se = block_sum(se, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = se;
}
// the balance pass, once per outer over all groups: x = f y with f = Q / (U - E) from sums = { U, E, Q } (f = 1 where that is not finite,
// U = E, or rebalance = 0), old <- x, and the block partials of Phi, P, ||x||^2, ||x - old||^2 (rows 0..3, as k_subcrit_reduce).  Every
// thread forms the same f; block 0 stores it in sums[3].
__global__ __launch_bounds__(256) void k_tr_balance(const double *__restrict__ Mf, const double *__restrict__ y, double *__restrict__ old,
                                                    const double *__restrict__ hx, const double *__restrict__ hy, const double *__restrict__ hz,
                                                    int nx, int ny, long N, long n, long ntot, double *sums, int rebalance,
                                                    double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    double f = 1.0;
    if (rebalance) {
        const double U = sums[0], E = sums[1], Q = sums[2];
        const double t = Q / (U - E);
        if (U != E && (t - t) == 0.0) f = t;
    }
    double sf = 0.0, sp = 0.0, sn = 0.0, sd = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ntot; i += gridDim.x * 256L) {
        const double v = f * y[i], d = v - old[i];
        sn += v * v; sd += d * d;
        old[i] = v;
        const long j = i - (i / n) * n;
        if (j < N) { sf += cell_measure(hx, hy, hz, nx, ny, j) * v; sp += Mf[i] * v; }
    }
    sf = block_sum(sf, sred); sp = block_sum(sp, sred); sn = block_sum(sn, sred); sd = block_sum(sd, sred);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sf; partials[stride + blockIdx.x] = sp;
        partials[2 * stride + blockIdx.x] = sn; partials[3 * stride + blockIdx.x] = sd;
        if (blockIdx.x == 0) sums[3] = f;
    }
}
// all precursor families in one pass, tf = sum_g Mf_g phi_g formed on the fly: c_i <- fam.a[i] c_i + fam.b[i] tf (a step: a = 1 / (1 +
// lambda_i dt), b = dt beta_i / (k0 (1 + lambda_i dt)); init = 1, the equilibrium at begin: c_i = fam.b[i] tf, c is not read).
// Row 0 of the partials: the precursor population, the sum of the DOF-0 rows of all c_i; row 1: P = the sum of the DOF-0 rows of tf.
__global__ __launch_bounds__(256) void k_tr_precursors(const double *__restrict__ Mf, const double *__restrict__ phi, double *__restrict__ c,
                                                       long N, long n, int ng, TrFamilies fam, int init, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    double sc = 0.0, sp = 0.0;
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n; j += gridDim.x * 256L) {
        double tf = 0.0;
        for (int g = 0; g < ng; ++g) tf += Mf[g * n + j] * phi[g * n + j];
        if (j < N) sp += tf;
        for (int i = 0; i < fam.n; ++i) {
            const double v = init ? fam.b[i] * tf : fam.a[i] * c[i * n + j] + fam.b[i] * tf;
            c[i * n + j] = v;
            if (j < N) sc += v;
        }
    }
    sc = block_sum(sc, sred); sp = block_sum(sp, sred);
    if (threadIdx.x == 0) { partials[blockIdx.x] = sc; partials[stride + blockIdx.x] = sp; }
}
// ---- adjoint-weighted kinetics parameters, nf_kinetics_params / nf_transient_kinetics ----------------------------------
// All bilinear forms of the point-kinetics balance in ONE streaming pass over the n DOF indices of a group: with w the adjoint flux,
// y_g = S_g phi_g (the Schur apply of the built operator, formed before this launch), tf = sum_g Mf_g phi_g, xw = sum_g chi_g w_g and
// xd = sum_g chi_d,g w_g (chi_d as in k_tr_chi), the rows of the partials are
//   0 production = sum xw tf    1 delayed_production = sum xd tf    2 removal_leakage = sum_g w_g y_g
//   3 scatter = sum_{g != g'} w_g Ms[g<-g'] phi_g' (the built blocks, Ms as k_tr_emission takes them)
//   4 amplitude = sum W sum_g w_g phi_g / v_g (ivel.v[g] = 1 / v_g)    5 + i  c_amp[i] = sum xd c_i   (i < nfam; c may be NULL with nfam = 0)
// Per index: w_g, phi_g, y_g, Mf_g of every group, chi_g of the cell, W, the non-empty scatter blocks and the nfam precursor vectors,
// each read once with consecutive lanes on consecutive doubles (phi_g' of a scatter term is the load of the group loop again); xw, xd, tf
// and the 5 + NF_PRECURSORS_MAX running sums stay in registers (the family loop is unrolled over its bound so that they do).  The cell
// of an index is carried along the grid stride (one modulo per thread, not one per index).  One share per block and sum, k_finalize adds them.
__global__ __launch_bounds__(256) void k_kin_forms(const double *__restrict__ w, const double *__restrict__ phi, const double *__restrict__ y,
                                                   const double *__restrict__ Mf, const double *__restrict__ chi, const double *__restrict__ W,
                                                   const double *const *__restrict__ Ms, const double *__restrict__ c, long N, long n, int ng,
                                                   TrGroups ivel, TrGroups chid, int per_cell, int nfam, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    double sp = 0.0, sd = 0.0, sl = 0.0, ss = 0.0, sa = 0.0, sc[NF_PRECURSORS_MAX];
#pragma unroll
    for (int i = 0; i < NF_PRECURSORS_MAX; ++i) sc[i] = 0.0;
    const long step = gridDim.x * 256L, estep = step % N;
    long j = blockIdx.x * 256L + threadIdx.x, e = j % N;
    for (; j < n; j += step) {
        double xw = 0.0, xd = 0.0, tf = 0.0, am = 0.0;
        for (int g = 0; g < ng; ++g) {
            const double wg = w[g * n + j], pg = phi[g * n + j], cg = chi[g * N + e];
            xw += cg * wg; xd += (per_cell ? cg : chid.v[g]) * wg;
            tf += Mf[g * n + j] * pg;
            sl += wg * y[g * n + j];
            am += ivel.v[g] * (wg * pg);
            for (int gp = 0; gp < ng; ++gp) {
                const double *M = Ms[g * ng + gp];
                if (gp == g || !M) continue;
                ss += wg * (M[j] * phi[gp * n + j]);
            }
        }
        sa += W[j] * am; sp += xw * tf; sd += xd * tf;
#pragma unroll
        for (int i = 0; i < NF_PRECURSORS_MAX; ++i)
            if (i < nfam) sc[i] += xd * c[i * n + j];
        e += estep; if (e >= N) e -= N;
    }
    sp = block_sum(sp, sred); sd = block_sum(sd, sred); sl = block_sum(sl, sred); ss = block_sum(ss, sred); sa = block_sum(sa, sred);
#pragma unroll
    for (int i = 0; i < NF_PRECURSORS_MAX; ++i)
        if (i < nfam) sc[i] = block_sum(sc[i], sred);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sp; partials[stride + blockIdx.x] = sd; partials[2 * stride + blockIdx.x] = sl;
        partials[3 * stride + blockIdx.x] = ss; partials[4 * stride + blockIdx.x] = sa;
#pragma unroll
        for (int i = 0; i < NF_PRECURSORS_MAX; ++i)
            if (i < nfam) partials[(5 + i) * stride + blockIdx.x] = sc[i];
    }
}
// phi /= norm, then ChebyshevAccel::operator() (src/solvers.cpp:720-756) with the step of cheb_next.  cur <- result; after mode 3 the
// caller swaps p0 / p1.
__global__ __launch_bounds__(256) void k_normalize_cheb(const double *__restrict__ raw, double *__restrict__ cur,
                                                        double *__restrict__ p0, double *__restrict__ p1, long ntot,
                                                        double norm, int do_norm, int mode, double ca, double cb)
{
    const ChebStep cs = { mode, ca, cb };
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ntot; i += gridDim.x * 256L) cur[i] = cheb_update(raw[i], do_norm, norm, cs, p0, p1, i);
}

// ---------------------------------------------------------------------------------------------
// Diagonal-Schur power iteration with the whole outer loop on the device (undivided RT0-P0 mesh, no CMFD): an outer
// iteration is ng pointwise group solves, one scalar kernel and one normalise kernel, all a few microseconds on the
// benchmark meshes, so a host round trip per outer would dominate.  The scalar logic of src/NeutFEM.cpp:1766-1802 and of
// ChebyshevAccel (src/solvers.cpp:720-756) lives in k_outer_logic; the host launches batches of outers and reads the
// state once per batch.  Kernels of outers queued behind the last one exit on `done`.
struct OuterState {
    double keff, norm, a, b;
    double tol_keff, tol_flux;
    ChebTable cheb;
    int mode, do_norm, it, cheb_it, swap, swap_next, max_outer;
    int done;                       // 0 running, 1 finished (converged or max_outer), 2 diverged
    int done_next;                  // the current outer is the last one: its normalise kernel still runs (:1780-1802)
};
// group g: rhs = chi_g tf / k + scatter (Gauss-Seidel), raw_g = S_inv rhs (:607-613), and this group's share of
// prod_new = sum M_f raw, |raw|^2, |raw - phi_old|^2 (:1766-1779) accumulated block-wise over the groups (g = 0 stores)
__global__ __launch_bounds__(256) void k_diag_group(ScatterArgs sa, int g, const double *__restrict__ chi, const double *__restrict__ tf,
                                                    const double *__restrict__ raw_all, const double *__restrict__ phi_old,
                                                    const double *__restrict__ sinv, const double *__restrict__ Mf, double *__restrict__ out,
                                                    long n, const OuterState *__restrict__ st, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    if (st->done || st->done_next) return;
    const double inv_k = 1.0 / st->keff;
    double sp = 0.0, sn = 0.0, sd = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        double v = inv_k * (chi[i] * tf[i]);
        for (int gp = 0; gp < sa.ng; ++gp) {
            if (gp == g || !sa.M[gp]) continue;
            const double *ph = gp < g ? raw_all : phi_old;
            v += sa.M[gp][i] * ph[gp * n + i];
        }
        const double r = sinv[i] * v, d = r - phi_old[g * n + i];
        out[i] = r;
        sp += Mf[i] * r; sn += r * r; sd += d * d;
    }
    sp = block_sum(sp, sred); sn = block_sum(sn, sred); sd = block_sum(sd, sred);
    if (threadIdx.x == 0) {
        double *p1 = partials + stride + blockIdx.x, *p2 = partials + 2 * stride + blockIdx.x, *p3 = partials + 3 * stride + blockIdx.x;
        if (g == 0) { *p1 = sp; *p2 = sn; *p3 = sd; } else { *p1 += sp; *p2 += sn; *p3 += sd; }
    }
}
// one block: sums of the four partial rows (row 0: prod_old from k_fission / k_normalize_fission), then the scalar logic
__global__ __launch_bounds__(256) void k_outer_logic(const double *__restrict__ partials, int cnt0, int cnt, long stride,
                                                     OuterState *__restrict__ st, double *__restrict__ hist_k,
                                                     double *__restrict__ hist_dk, double *__restrict__ hist_dphi)
{
    __shared__ double sred[4];
    if (st->done) return;
    if (st->done_next) { if (threadIdx.x == 0) st->done = 1; return; }
    double tot[4];
    for (int q = 0; q < 4; ++q) {
        double s = 0.0;
        const int c = q == 0 ? cnt0 : cnt;
        for (int i = threadIdx.x; i < c; i += 256) s += partials[q * stride + i];
        tot[q] = block_sum(s, sred);
    }
    if (threadIdx.x != 0) return;
    const int it = st->it;
    const OuterStep os = outer_step(st->keff, it, tot[0], tot[1], tot[2], tot[3]);
    st->keff = os.keff;
    hist_k[it] = os.keff; hist_dk[it] = os.dk; hist_dphi[it] = os.dphi;
    if (!os.finite) { st->it = it + 1; st->done = 2; return; }
    int cheb_it = st->cheb_it;
    const ChebStep cs = cheb_next(cheb_it, st->cheb, it >= 2);  // src/solvers.cpp:720-756
    st->cheb_it = cheb_it;
    st->swap = st->swap_next;                                   // orientation of (p0, p1) for this outer's normalise kernel
    st->swap_next = st->swap ^ (cs.mode == 3 ? 1 : 0);
    st->mode = cs.mode; st->a = cs.a; st->b = cs.b; st->norm = os.norm; st->do_norm = os.do_norm ? 1 : 0;
    st->it = it + 1;
    if (outer_converged(os.dk, os.dphi, st->tol_keff, st->tol_flux) || it + 1 >= st->max_outer) st->done_next = 1;   // :1799-1802
}
// phi_g = Chebyshev(raw_g / norm) for every group of a cell, and the next outer's total_fiss + prod_old partials (:1700-1707)
__global__ __launch_bounds__(256) void k_normalize_fission(const double *__restrict__ raw, double *__restrict__ cur,
                                                           double *__restrict__ p0, double *__restrict__ p1,
                                                           const double *__restrict__ Mf, int ng, long n,
                                                           const OuterState *__restrict__ st, double *__restrict__ tf,
                                                           double *__restrict__ partials)
{
    __shared__ double sred[4];
    if (st->done) return;
    const double norm = st->norm;
    const int do_norm = st->do_norm;
    const ChebStep cs = { st->mode, st->a, st->b };
    double *pa = st->swap ? p1 : p0, *pb = st->swap ? p0 : p1;
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        double t = 0.0;
        for (int g = 0; g < ng; ++g) {
            const long j = g * n + i;
            const double v = cheb_update(raw[j], do_norm, norm, cs, pa, pb, j);
            cur[j] = v;
            t += Mf[j] * v;
        }
        tf[i] = t; s += t;
    }
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------
// Resident solve: the whole SolveKeff (full Schur path: power iteration, Gauss-Seidel group sweep, CG, Chebyshev;
// src/NeutFEM.cpp:1627-1815, src/solvers.cpp:577-636, 664-756) of a SMALL undivided mesh in ONE workgroup and ONE launch.
// The reference's own benchmark meshes (IAEA-2D 38x38, KOEBERG 34x34, every coarse-mesh initialisation) are a few thousand
// unknowns: as separate launches a CG iteration is 4 x ~5 us of launch and cross-chip latency for ~100 KB of data.  Here every
// phase is separated by a workgroup barrier only; the direction passes are the same device functions as the big-mesh kernels
// (schur_x_task, schur_s_tile: identical per-cell arithmetic), run over "virtual" tiles; reductions are fixed-order
// (thread-strided, then wave, then across waves), so runs are reproducible; every thread derives the same scalars from them.
struct ResidentArgs {
    Geom G; int ng, dim, nmodes; long N, nphi;
    ModeArgs ma[3]; ModeTab mt[3];          // per direction, mode 0, group 0, x -> p, y -> q; Cd and D advance with the group
    const double *L[3], *DR[3], *D0[3]; long nlines[3];
    const double *Mf, *Chi; const double *const *Ms;             // Ms: ng*ng table of scatter diagonals (null = empty block, :1722)
    double *phi, *raw, *p0, *p1, *tf, *r, *p, *q;
    int lpl_log2, ntask_x;
    int n[2], TX[2], NSEG[2], gx[2], gy[2]; long sl[2], ostride[2];
    double keff0, tol_keff, tol_flux, cg_tol; int cg_max, max_outer;
    ChebTable cheb;
    double *hist; int *hist_cg; ResidentOut *out;
    // LDS residency (host plan, greedy by priority): bit 0 p, 1 q, 2 r, 3 x_sol, 4+2d L[d], 5+2d DR[d], 10 C diagonal.  One CU
    // moves ~10 B/cycle to and from L2 but 128 B/cycle to and from LDS, and a barrier no longer waits for global store acks.
    const double *Cd0; int lds_mask;
    // Line-per-lane variants (k_resident_keff<.., NB, PITCH != 0>): first lane slot of every direction (each direction starts on a
    // wavefront boundary; slot0[3] = number of slots), and whether a direction's lines are swept by pairs of lanes
    int slot0[4], tw[3];                                         // tw: two lanes per line in that direction (lines of >= 4 cells)
    // the same for RT_k-P_m with bubble moments (k_resident_keff<.., NB > 0, -1>): cell pitch, the moment index of every (direction,
    // transverse mode, along-index), and per (moment, direction) the factor T_a G_l^2 / M^bb_l of the bubble's diagonal term (0 when
    // the moment has no bubble in that direction), which is folded into the C diagonal once per group
    int PC, mom[3][9][3]; double diagc[27][3];
};
__device__ __forceinline__ double block_total(double v, double *sred)     // fixed-order sum over the block, result in every thread
{
    v = block_sum(v, sred);
    if (threadIdx.x == 0) sred[0] = v;
    __syncthreads();
    v = sred[0];
    __syncthreads();
    return v;
}
// One barrier instead of four: every wavefront leaves its partial in the buffer of the given parity and every thread adds the (at most 8)
// partials in the same fixed order.  Two reductions of the same parity must be separated by a barrier (the CG loop alternates).
__device__ __forceinline__ double block_total_1b(double v, double *sred, int parity)
{
    v = wave_sum(v);
    double *b = sred + parity * 8;
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) b[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += b[w];
    return s;
}
// RT0-P0 on a mesh that lives in LDS: one lane per line, both sweeps serial along the line -- no scans, no barriers.  For lines of a few
// dozen cells the dependent chain of n multiply-adds per sweep is several times shorter than the instruction stream of the segmented
// scans (in-kernel stamps, IAEA-2D 38 x 38: 10.9 k + 6.2 k cycles for the x and y passes of the scan kernels).
//   forward  z_{c+1} = (x_c - x_{c+1}) - L_c z_c, z_0 = -x_0, w_f = z_f / d_f ; backward u_f = w_f - L_f u_{f+1} ; out_c = Ta (u_{c+1} - u_c)
// blk: the direction's block of three arrays at a compile-time pitch -- L, 1/d, out -- so that one address register serves all three
// (LDS instructions carry a 16-bit byte offset).  The n - 1 cells that have an upper neighbour go in unpredicated pieces of 8 / 4 / 2 / 1
// cells (a predicated or clamped load costs more instructions than the arithmetic), the last cell on its own.
typedef __attribute__((address_space(3))) double lds_f64;      // explicit LDS pointers: ds_read / ds_write with 32-bit addresses, not flat accesses
// Three per-direction values as named members.  A local array T v[3] that is indexed by a run-time direction anywhere (or through a chain
// d == 0 ? v[0] : ..., which the optimiser folds back into v[d]) is kept in scratch memory for the whole kernel, and every use inside the
// CG loop becomes a scratch load in front of the dependent LDS access.
template <class T> struct Tri {
    T a, b, c;
    __device__ __forceinline__ T operator[](int d) const { return d == 0 ? a : d == 1 ? b : c; }
    __device__ __forceinline__ void set(int d, T v) { if (d == 0) a = v; else if (d == 1) b = v; else c = v; }
};
template <int CH, int PITCH>
__device__ __forceinline__ void serial_fwd(const lds_f64 *&xp, lds_f64 *&bp, int sl, double &z, double &xc)
{
    double xv[CH + 1], Lv[CH], Rv[CH];
    xv[0] = xc;
#pragma unroll
    for (int i = 0; i < CH; ++i) { Lv[i] = bp[i * sl]; Rv[i] = bp[i * sl + PITCH]; xv[i + 1] = xp[(i + 1) * sl]; }
#pragma unroll
    for (int i = 0; i < CH; ++i) { z = (xv[i] - xv[i + 1]) - Lv[i] * z; bp[i * sl + 2 * PITCH] = z * Rv[i]; }
    xc = xv[CH]; xp += CH * sl; bp += CH * sl;
}
template <int CH, int PITCH>
__device__ __forceinline__ void serial_bwd(lds_f64 *&bp, int sl, double Ta, double &u2, double &Ln)
{
    double wv[CH], Lv[CH];
    bp -= CH * sl;
#pragma unroll
    for (int i = 0; i < CH; ++i) { wv[i] = bp[i * sl + 2 * PITCH]; Lv[i] = bp[i * sl]; }
#pragma unroll
    for (int i = CH - 1; i >= 0; --i) {
        const double u1 = wv[i] - Ln * u2;                       // u_{c+1}
        bp[(i + 1) * sl + 2 * PITCH] = Ta * (u2 - u1);           // cell c + 1
        u2 = u1; Ln = Lv[i];
    }
}
// Two lanes per line ("burn at both ends"): the even lane eliminates from face 0 up to the middle face k = n / 2, the odd lane -- on the
// mirrored line, with the factors of the mirrored elimination in its cells' slots (serial_twist_factors) -- from face n down to it; they
// meet in u_k = (b_k - l_{k-1} z_{k-1} - l~ z~) / d'_k and substitute outwards.  Mirroring turns b into -b and u into -u, the outputs
// T_a (u_{c+1} - u_c) come out the same, so both lanes run the same code with `cnt` own cells, a stride of opposite sign and their own
// first pivot.  Half the dependent chain, half the instructions per wavefront.
__device__ __forceinline__ double quad_swap(double v)            // value of the partner lane (lane ^ 1)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0xB1, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0xB1, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double pair_even(double v)            // value of the even lane of the pair
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0xA0, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0xA0, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
template <int PITCH>
__device__ __forceinline__ void serial_line_rt0(const lds_f64 *x, lds_f64 *blk, double d0, double dm, double Ta, int cnt, int base, int sl,
                                                bool two_sided, bool top)
{
    const lds_f64 *xp = x + base; lds_f64 *bp = blk + base;
    double xc = xp[0], z = -xc;
    const double w0 = z * d0;
    const int m = cnt - 1;
    for (int k = 0; k < (m >> 3); ++k) serial_fwd<8, PITCH>(xp, bp, sl, z, xc);
    if (m & 4) serial_fwd<4, PITCH>(xp, bp, sl, z, xc);
    if (m & 2) serial_fwd<2, PITCH>(xp, bp, sl, z, xc);
    if (m & 1) serial_fwd<1, PITCH>(xp, bp, sl, z, xc);
    double Ln = bp[0], u2;
    if (two_sided) {
        const double Pown = Ln * z, b = xc - xp[sl];             // xp[sl]: the partner's last cell
        const double Poth = quad_swap(Pown);
        const double um = ((b + Poth) - Pown) * dm;
        const double ut = pair_even(um);                         // one value for both halves
        u2 = top ? ut : -ut;
    } else {
        z = xc - Ln * z;                                         // the last cell: nothing above it
        u2 = z * bp[PITCH];                                      // u_n = w_n (L_n = 0)
    }
    if (m & 1) serial_bwd<1, PITCH>(bp, sl, Ta, u2, Ln);
    if (m & 2) serial_bwd<2, PITCH>(bp, sl, Ta, u2, Ln);
    if (m & 4) serial_bwd<4, PITCH>(bp, sl, Ta, u2, Ln);
    for (int k = 0; k < (m >> 3); ++k) serial_bwd<8, PITCH>(bp, sl, Ta, u2, Ln);
    const double u0 = w0 - Ln * u2;
    bp[2 * PITCH] = Ta * (u2 - u0);
}
// Factors of the mirrored elimination for the upper part of a line (cells k .. n-1), from the stored top-down factors: d_f = 1 / (1/d_f),
// e_c = l_c d_c, t_f = d_f + l_{f-1} e_{f-1}; then d^_n = t_n, l~_f = e_f / d^_{f+1}, d^_f = t_f - l~_f e_f downwards.  Cell c gets l~_c in
// its L slot and 1 / d^_c in its 1/d slot (what the mirrored sweep expects there); returns 1 / d^_n, and 1 / d'_k of the middle face
// (d'_k = d_k - l~_k e_k) through dm.  L: the line's first cell, oR: offset of the 1/d slots.
__device__ __forceinline__ double serial_twist_factors(lds_f64 *L, int oR, double d0inv, int n, int k, int sl, double &dm)
{
    auto dpiv = [&](int f) { return 1.0 / (f == 0 ? d0inv : (double)L[(f - 1) * sl + oR]); };   // standard pivot of face f
    double dlo = dpiv(n - 1), elo = L[(n - 1) * sl] * dlo;       // d_{n-1}, e_{n-1}
    double dhat = dpiv(n) + L[(n - 1) * sl] * elo;               // t_n
    const double first = 1.0 / dhat;
    for (int f = n - 1; f > k; --f) {                            // face f: cell f holds l~_f and 1 / d^_f
        const double dlo2 = dpiv(f - 1), elo2 = L[(f - 1) * sl] * dlo2;
        const double tf = dlo + L[(f - 1) * sl] * elo2;
        const double lt = elo / dhat;
        L[f * sl] = lt;
        dhat = tf - lt * elo;
        L[f * sl + oR] = 1.0 / dhat;
        dlo = dlo2; elo = elo2;
    }
    const double lk = elo / dhat;                                // dlo = d_k, elo = e_k here
    L[k * sl] = lk;
    dm = 1.0 / (dlo - lk * elo);
    return first;
}
// The same for RT_k-P_m with NB bubble moments (formulas above ModeArgs).  x / y: moment 0 of the line's transverse mode at the first cell,
// o1 / o2: offsets of the along-moments 1 and 2; L at the first cell, 1/d at offset oR.  The bubbles' own diagonal term
// T_a G_l^2 x_{l+1} / (M^bb_l c_e) is not formed here: it sits in the thread-private C diagonal of the cell pass.
struct HiConst { double eL[2], eR[2], Gc[2]; };
template <int NB>
__device__ __forceinline__ void hi_faces(double x0, double x1, double x2, const HiConst &c, double &xL, double &xR)
{
    double pl = 0.0, pr = 0.0;
    if (NB > 0) { const double g = c.Gc[0] * x1; pl += c.eL[0] * g; pr += c.eR[0] * g; }
    if (NB > 1) { const double g = c.Gc[1] * x2; pl += c.eL[1] * g; pr += c.eR[1] * g; }
    xL = x0 + pl; xR = x0 - pr;
}
template <int CH, int NB>
__device__ __forceinline__ void hi_fwd(const lds_f64 *&xp, int o1, int o2, const lds_f64 *&Lp, int oR, lds_f64 *&wp, int sl, double &z, double &xRc,
                                       const HiConst &c)
{
    double x0[CH], x1[CH], x2[CH], Lv[CH], Rv[CH];              // xp: the cell above the current one; Lp, wp: the current cell
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        x0[i] = xp[i * sl]; x1[i] = NB > 0 ? xp[i * sl + o1] : 0.0; x2[i] = NB > 1 ? xp[i * sl + o2] : 0.0;
        Lv[i] = Lp[i * sl]; Rv[i] = Lp[i * sl + oR];
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        double xLn, xRn;
        hi_faces<NB>(x0[i], x1[i], x2[i], c, xLn, xRn);
        z = (xRc - xLn) - Lv[i] * z; wp[i * sl] = z * Rv[i]; xRc = xRn;
    }
    xp += CH * sl; Lp += CH * sl; wp += CH * sl;
}
template <int NB>
__device__ __forceinline__ void hi_emit(lds_f64 *yp, int o1, int o2, double Ta, double lo, double hi, const HiConst &c)
{
    yp[0] = Ta * (hi - lo);
    if (NB > 0) yp[o1] = -(Ta * c.Gc[0]) * (c.eL[0] * lo + c.eR[0] * hi);
    if (NB > 1) yp[o2] = -(Ta * c.Gc[1]) * (c.eL[1] * lo + c.eR[1] * hi);
}
template <int CH, int NB>
__device__ __forceinline__ void hi_bwd(const lds_f64 *&Lp, lds_f64 *&yp, int o1, int o2, int sl, double Ta, double &u2, double &Ln, const HiConst &c)
{
    double wv[CH], Lv[CH];
    Lp -= CH * sl; yp -= CH * sl;
#pragma unroll
    for (int i = 0; i < CH; ++i) { wv[i] = yp[i * sl]; Lv[i] = Lp[i * sl]; }
#pragma unroll
    for (int i = CH - 1; i >= 0; --i) {
        const double u1 = wv[i] - Ln * u2;                       // u_{c+1}: lower face of cell c + 1, u2 its upper face
        hi_emit<NB>(yp + (i + 1) * sl, o1, o2, Ta, u1, u2, c);
        u2 = u1; Ln = Lv[i];
    }
}
// cnt own cells; two_sided: see serial_line_rt0 -- the mirrored half sees the odd along-moment with the opposite sign, which is the
// caller's business (HiConst::Gc[0] negated: it multiplies x_1 on the way in and y_1 on the way out)
template <int NB>
__device__ __forceinline__ void serial_line_hi(const lds_f64 *x, int o1, int o2, const lds_f64 *L, int oR, lds_f64 *y, double d0, double dm, double Ta,
                                               const HiConst &c, int cnt, int sl, bool two_sided, bool top)
{
    const lds_f64 *xp = x + sl, *Lp = L; lds_f64 *wp = y;
    double xL0, xRc;
    hi_faces<NB>(x[0], NB > 0 ? x[o1] : 0.0, NB > 1 ? x[o2] : 0.0, c, xL0, xRc);
    double z = -xL0;
    const double w0 = z * d0;
    const int m = cnt - 1;
    for (int k = 0; k < (m >> 2); ++k) hi_fwd<4, NB>(xp, o1, o2, Lp, oR, wp, sl, z, xRc, c);
    if (m & 2) hi_fwd<2, NB>(xp, o1, o2, Lp, oR, wp, sl, z, xRc, c);
    if (m & 1) hi_fwd<1, NB>(xp, o1, o2, Lp, oR, wp, sl, z, xRc, c);
    double Ln = Lp[0], u2;
    if (two_sided) {
        double xLn, xRn;
        hi_faces<NB>(xp[0], NB > 0 ? xp[o1] : 0.0, NB > 1 ? xp[o2] : 0.0, c, xLn, xRn);   // the partner's last cell, seen from this side
        const double Pown = Ln * z, b = xRc - xLn;
        const double Poth = quad_swap(Pown);
        const double um = ((b + Poth) - Pown) * dm;
        const double ut = pair_even(um);
        u2 = top ? ut : -ut;
    } else {
        z = xRc - Ln * z;                                        // the last cell: nothing above it
        u2 = z * Lp[oR];
    }
    lds_f64 *yp = wp;
    if (m & 1) hi_bwd<1, NB>(Lp, yp, o1, o2, sl, Ta, u2, Ln, c);
    if (m & 2) hi_bwd<2, NB>(Lp, yp, o1, o2, sl, Ta, u2, Ln, c);
    for (int k = 0; k < (m >> 2); ++k) hi_bwd<4, NB>(Lp, yp, o1, o2, sl, Ta, u2, Ln, c);
    const double u0 = w0 - Ln * u2;
    hi_emit<NB>(yp, o1, o2, Ta, u0, u2, c);
}
// all tiles of one y / z pass, nconc = blockDim / (TX NSEG) of them side by side; every thread runs every round (barriers inside)
template <int SEG, int DIR, int NB>
__device__ __forceinline__ double resident_s_pass(const ResidentArgs &A, int r, const ModeArgs &mad, const double *Ld, const double *DRd, int g, double *sm,
                                                  const SlabArgs &sa0, const CgFuse &fz)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int T = A.TX[r] * A.NSEG[r];
    const int nconc = nt / T, slot = tid / T, ltid = tid - slot * T;
    const int ntiles = A.gx[r] * A.gy[r] * A.nmodes;
    double *smt = sm + (slot < nconc ? slot : 0) * (4 * T + (A.NSEG[r] >= 64 ? 5 : 1) * A.TX[r]);   // padded rows when the wavefront scan is on
    double dot = 0.0;
    for (int t0 = 0; t0 < ntiles; t0 += nconc) {
        const int t = t0 + slot;
        const bool act = slot < nconc && t < ntiles;
        const unsigned tt = act ? t : 0;
        const unsigned bx = tt % A.gx[r], by = (tt / A.gx[r]) % A.gy[r], bz = tt / (A.gx[r] * A.gy[r]);
        const ModeArgs ma = select_mode(mad, A.mt[DIR], bz, NB + 1);
        dot += schur_s_tile<SEG, DIR, false, NB>(ma, A.G, Ld, DRd, A.D0[DIR] + g * A.nlines[DIR], A.n[r], A.sl[r], A.ostride[r],
                                                 A.G.nx, A.TX[r], A.NSEG[r], bx, by, bz, A.gy[r], ltid, act, smt, sa0, fz, false, false, 0.0, 0.0, true);
        __syncthreads();                                         // the tile's scan arrays are reused by the next round
    }
    return dot;
}
// The solve of one workgroup; no blockIdx / gridDim below, nothing shared with another workgroup.  Two entries call it: k_resident_keff
// (one mesh, the struct a kernel argument) and k_resident_keff_batch (one mesh per workgroup, the structs in a device array).
template <bool VEC, int NB, int PITCH>                            // PITCH > 0: the line-per-lane variant (RT0-P0, everything in LDS)
__device__ __forceinline__ void resident_keff_body(const ResidentArgs &A)
{
    constexpr bool SERIAL = PITCH > 0;                             // RT0-P0 line-per-lane variant
    constexpr bool SERH = PITCH < 0;                               // line-per-lane variant with bubble moments
    static_assert(!SERIAL || NB == 0, "a compile-time pitch is the RT0-P0 variant");
    static_assert(!SERH || NB > 0, "the run-time pitch variant is for NB > 0");
    constexpr int SEG = NB > 0 ? 4 : 8;
    extern __shared__ double sm[];
    const int scr = (SERIAL || SERH) ? 0 : 5 * (int)blockDim.x;   // scratch of the tiled passes
    double *sred = sm + scr + 64;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, nw = nt >> 6;
    const int ng = A.ng; const long N = A.N, NP = A.nphi, NT = NP * ng;
    // the lane plan's per-direction values by name (Tri, below): read here once, so that no chain d == 0 ? A.v[0] : ... is left that the
    // optimiser could turn into a choice between addresses inside A -- with those the struct is no longer taken apart and goes to scratch whole
    const Tri<int> aS0 = { A.slot0[0], A.slot0[1], A.slot0[2] }, aTw = { A.tw[0], A.tw[1], A.tw[2] }, aNl = { (int)A.nlines[0], (int)A.nlines[1], (int)A.nlines[2] };
    const Tri<double> aTa = { A.ma[0].Ta, A.ma[1].Ta, A.ma[2].Ta };
    const int aSlots = A.slot0[3];
    SlabArgs sa0; sa0.if_lo = sa0.if_hi = sa0.mode = sa0.xcd = sa0.wsmin = sa0.fold = sa0.noacc = 0; sa0.yadd = nullptr; sa0.alo = sa0.ahi = sa0.ulo = sa0.uhi = sa0.rlo = sa0.rhi = sa0.sinv_lo = sa0.sinv_hi = nullptr; sa0.clo = sa0.chi = sa0.jz = sa0.jzb = nullptr; sa0.nfa = 1; sa0.ni = 0;
    // vectors and factors that fit are kept in LDS behind the scratch area (ResidentArgs::lds_mask); the rest stays in global memory
    double *lds = sm + scr + 64 + 16;
    long lo = 0;
    auto carve = [&](int bit, long n) -> double * { if (!((A.lds_mask >> bit) & 1)) return nullptr; double *q_ = lds + lo; lo += (n + 1) & ~1L; return q_; };
    double *vp = carve(0, NP), *vq = carve(1, NP), *vr = carve(2, NP), *vx = carve(3, NP);
    double *fL[3], *fR[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { fL[d] = carve(4 + 2 * d, N); fR[d] = carve(5 + 2 * d, N); }
    double *fC = carve(10, NP);
    // Line-per-lane variant.  LDS: p, then per direction a block {L, 1/d, contribution} at pitch PITCH and the first pivots of its lines;
    // rows padded to an odd length nxp (x lines: lane = line, so the lanes of a wavefront are nxp doubles apart -- odd means no bank
    // conflicts; an even nx = 38 gave 3-way conflicts on every access and an LDS-bound sweep).  Every thread owns the KC = PITCH / 512
    // padded cells tid + 512 k for the whole solve and keeps their r, x_sol and C diagonal in registers; cells of the padding and beyond
    // the mesh hold zeros everywhere, so nothing below is predicated.
    constexpr int KC = SERIAL ? PITCH / 512 : 1;
    lds_f64 *lp = nullptr; Tri<lds_f64 *> lb = { nullptr, nullptr, nullptr }; Tri<const lds_f64 *> lD = { nullptr, nullptr, nullptr };
    Tri<lds_f64 *> lDm = { nullptr, nullptr, nullptr }, lDr = { nullptr, nullptr, nullptr };   // 1 / d'_k and 1 / d^_n per line (two-sided sweeps)
    int gi[KC], nxp = 0;
    if (SERIAL) {
        nxp = A.G.nx | 1;
        lp = (lds_f64 *)lds; lo = PITCH;
#pragma unroll
        for (int d = 0; d < 3; ++d) if (d < A.dim) { lb.set(d, (lds_f64 *)(lds + lo)); lo += 3 * PITCH; }
#pragma unroll
        for (int d = 0; d < 3; ++d) if (d < A.dim) {
            const long nl2 = (A.nlines[d] + 1) & ~1L;
            lD.set(d, (const lds_f64 *)(lds + lo)); lDm.set(d, (lds_f64 *)(lds + lo + nl2)); lDr.set(d, (lds_f64 *)(lds + lo + 2 * nl2)); lo += 3 * nl2;
        }
        const int Np = nxp * A.G.ny * A.G.nz;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int ip = tid + k * 512, row = ip / nxp, ix = ip - row * nxp;
            gi[k] = (ip < Np && ix < A.G.nx) ? row * A.G.nx + ix : -1;
            lp[ip] = 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) if (d < A.dim) lb[d][2 * PITCH + ip] = 0.0;
        }
    }
    // Higher orders: DOF j = moment * PC + padded cell; p and one contribution vector per direction (nloc PC each), {L, 1/d} per
    // direction (PC each), first pivots; small tables (moment indices, T_a, diagonal factors) in LDS because a dynamically indexed
    // kernel argument would move the whole argument struct to scratch.  Every thread owns the DOFs tid + 512 k, k < KD.
    constexpr int KD = SERH ? 10 : 1;
    lds_f64 *hp = nullptr; Tri<lds_f64 *> hc = { nullptr, nullptr, nullptr }, hL = { nullptr, nullptr, nullptr }, hD = { nullptr, nullptr, nullptr };
    Tri<lds_f64 *> hDm = { nullptr, nullptr, nullptr }, hDr = { nullptr, nullptr, nullptr };
    lds_f64 *tTa = nullptr, *tDg = nullptr; __attribute__((address_space(3))) int *tMom = nullptr;
    int gj[KD], hPC = 0, hNPp = 0, hNp = 0;
    if (SERH) {
        nxp = A.G.nx | 1; hPC = A.PC; hNp = nxp * A.G.ny * A.G.nz;
        const int nloc = (int)(NP / N); hNPp = nloc * hPC;
        tTa = (lds_f64 *)lds; tDg = tTa + 32; tMom = (__attribute__((address_space(3))) int *)(tDg + 96); lo = 32 + 96 + 48;
        hp = (lds_f64 *)(lds + lo); lo += hNPp;
#pragma unroll
        for (int d = 0; d < 3; ++d) if (d < A.dim) { hc.set(d, (lds_f64 *)(lds + lo)); lo += hNPp; }
#pragma unroll
        for (int d = 0; d < 3; ++d) if (d < A.dim) { hL.set(d, (lds_f64 *)(lds + lo)); lo += 2 * hPC; }
#pragma unroll
        for (int d = 0; d < 3; ++d) if (d < A.dim) {
            const long nl2 = (A.nlines[d] + 1) & ~1L;
            lds_f64 *const b_ = (lds_f64 *)(lds + lo);
            hD.set(d, b_); hDm.set(d, b_ + nl2); hDr.set(d, b_ + 2 * nl2); lo += 3 * nl2;
        }
        if (tid < 27) { const int d = tid / 9, m = tid % 9; tTa[tid] = A.mt[d].n > 1 ? A.mt[d].Ta[m] : A.ma[d].Ta; }
        if (tid < 81) { tDg[tid] = A.diagc[tid / 3][tid % 3]; tMom[tid] = A.mom[tid / 27][(tid / 3) % 9][tid % 3]; }
#pragma unroll
        for (int k = 0; k < KD; ++k) {
            const int j = tid + k * 512, mo = j / hPC, ip = j - mo * hPC, row = ip / nxp, ix = ip - row * nxp;
            gj[k] = (j < hNPp && ip < hNp && ix < A.G.nx) ? mo * (int)N + row * A.G.nx + ix : -1;
            if (j < hNPp) { hp[j] = 0.0; hc[0][j] = 0.0; if (A.dim >= 2) hc[1][j] = 0.0; if (A.dim == 3) hc[2][j] = 0.0; }
        }
        __syncthreads();
    }
    double *const wp = vp ? vp : A.p, *const wq = vq ? vq : A.q, *const wr = vr ? vr : A.r;
    double keff = A.keff0;
    int cheb_it = 0, n_outer = 0, status = 0, cg_total = 0;
    double *pa = A.p0, *pb = A.p1;
    for (int it = 0; it < A.max_outer; ++it) {
        // total_fiss and prod_old (:1700-1707)
        double s = 0.0;
        for (long i = tid; i < NP; i += nt) {
            double v = 0.0;
            for (int g = 0; g < ng; ++g) v += A.Mf[g * NP + i] * A.phi[g * NP + i];
            A.tf[i] = v; s += v;
        }
        const double prod_old = block_total(s, sred);
        const double inv_k = 1.0 / keff;
        for (int g = 0; g < ng; ++g) {
            if constexpr (SERH) {
                double *const graw = A.raw + (long)g * NP;
                double rv[KD], xv[KD], cv[KD], pv[KD];
                const int nx = A.G.nx, ny = A.G.ny, n_ = (int)N;
                // this group's factors and first pivots
#pragma unroll
                for (int d = 0; d < 3; ++d) if (d < A.dim) {
                    for (int ip = tid; ip < hPC; ip += nt) {
                        const int row = ip / nxp, ix = ip - row * nxp;
                        const bool ok = ip < hNp && ix < nx;
                        const long e = g * N + row * nx + ix;
                        hL[d][ip] = ok ? A.L[d][e] : 0.0; hL[d][hPC + ip] = ok ? A.DR[d][e] : 0.0;
                    }
                    for (int i = tid; i < (int)A.nlines[d]; i += nt) hD[d][i] = A.D0[d][g * A.nlines[d] + i];
                }
                // two-sided directions: mirrored factors for the upper half of every line (one thread per line; the modes share them)
                __syncthreads();
#pragma unroll
                for (int d = 0; d < 3; ++d) if (d < A.dim && A.tw[d]) {
                    for (int l = tid; l < (int)A.nlines[d]; l += nt) {
                        const int base = d == 0 ? l * nxp : d == 1 ? (l / nx) * nxp * ny + l % nx : (l / nx) * nxp + l % nx;
                        const int sl = d == 0 ? 1 : d == 1 ? nxp : nxp * ny, n = d == 0 ? nx : d == 1 ? ny : A.G.nz;
                        double dm;
                        hDr[d][l] = serial_twist_factors(hL[d] + base, hPC, hD[d][l], n, n / 2, sl, dm);
                        hDm[d][l] = dm;
                    }
                }
                // rhs (:1716-1726), CG start (src/solvers.cpp:583-592); C diagonal + the bubbles' diagonal terms of every direction
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < KD; ++k) {
                    double v = 0.0; cv[k] = 0.0;
                    if (gj[k] >= 0) {
                        const int i = gj[k], mo = i / n_, e = i - mo * n_;
                        const double chv = A.Chi[g * N + e] * inv_k;
                        v = fabs(chv) < 1e-14 ? 0.0 : chv * A.tf[i];
                        for (int gp = 0; gp < ng; ++gp) {
                            const double *M = A.Ms[g * ng + gp];
                            if (gp == g || !M) continue;
                            v += M[i] * (gp < g ? A.raw : A.phi)[gp * NP + i];
                        }
                        const int ex = e % nx, ey = (e / nx) % ny, ez = e / (nx * ny);
                        const double Dc = A.ma[0].D[g * N + e];
                        double cd = A.Cd0[g * NP + i];
                        for (int d = 0; d < A.dim; ++d) { const double f = tDg[mo * 3 + d]; if (f != 0.0) cd += f * (Dc / geom_factor(A.G, d, ex, ey, ez)); }
                        cv[k] = cd;
                    }
                    rv[k] = v; pv[k] = v; xv[k] = 0.0; s += v * v;
                    if (tid + k * 512 < hNPp) hp[tid + k * 512] = v;
                }
                double rr = block_total(s, sred);
                const double rhs_norm = sqrt(rr), tol_sq = A.cg_tol * A.cg_tol * rhs_norm * rhs_norm;
                int its = 0;
                HiConst hcst;
                for (int l = 0; l < 2; ++l) { hcst.eL[l] = A.ma[0].eL[l]; hcst.eR[l] = A.ma[0].eR[l]; hcst.Gc[l] = A.ma[0].Gc[l]; }
                const int nm = A.nmodes;
                // which (direction, mode, line half) a lane slot sweeps; slot `tid` is decoded once per group
                struct LaneLine { bool ok, tw, top; int cnt, sl, o1, o2; double d0, dm, Ta; const lds_f64 *x, *L; lds_f64 *y; HiConst c; };
                auto lane_line = [&](int sl_) -> LaneLine {
                    LaneLine o; o.ok = false; o.tw = o.top = false; o.cnt = o.sl = o.o1 = o.o2 = 0; o.d0 = o.dm = o.Ta = 0.0; o.x = o.L = hp; o.y = hc[0]; o.c = hcst;
                    if (sl_ >= aSlots) return o;
                    const int d = sl_ >= aS0.c ? 2 : sl_ >= aS0.b ? 1 : 0;
                    const int nl = aNl[d];
                    const int twd = aTw[d];
                    const int rem = sl_ - (aS0[d]);
                    const int lane_l = twd ? rem >> 1 : rem;
                    const int mode = lane_l / nl, l = lane_l - mode * nl;
                    if (mode >= nm) return o;
                    o.ok = true; o.tw = twd != 0; o.top = !twd || !(rem & 1);
                    const int m0 = tMom[(d * 9 + mode) * 3];
                    o.o1 = (tMom[(d * 9 + mode) * 3 + 1] - m0) * hPC; o.o2 = NB > 1 ? (tMom[(d * 9 + mode) * 3 + 2] - m0) * hPC : 0;
                    const int base0 = d == 0 ? l * nxp : d == 1 ? (l / nx) * nxp * ny + l % nx : (l / nx) * nxp + l % nx;
                    const int sl0 = d == 0 ? 1 : d == 1 ? nxp : nxp * ny, n = d == 0 ? nx : d == 1 ? ny : A.G.nz;
                    o.cnt = !twd ? n : o.top ? n / 2 : n - n / 2; o.sl = o.top ? sl0 : -sl0;
                    const int base = o.top ? base0 : base0 + (n - 1) * sl0;
                    o.x = hp + m0 * hPC + base; o.L = (d == 0 ? hL[0] : d == 1 ? hL[1] : hL[2]) + base; o.y = (d == 0 ? hc[0] : d == 1 ? hc[1] : hc[2]) + m0 * hPC + base;
                    o.d0 = o.top ? (d == 0 ? hD[0] : d == 1 ? hD[1] : hD[2])[l] : (d == 0 ? hDr[0] : d == 1 ? hDr[1] : hDr[2])[l];
                    o.dm = twd ? (d == 0 ? hDm[0] : d == 1 ? hDm[1] : hDm[2])[l] : 0.0;
                    o.Ta = tTa[d * 9 + mode];
                    if (!o.top) o.c.Gc[0] = -o.c.Gc[0];          // mirrored line: the odd along-moment changes sign
                    return o;
                };
                const LaneLine my = lane_line(tid);
                while (its < A.cg_max) {
#ifdef NF_STAMPS
                    long long ts0 = (long long)__builtin_readcyclecounter();
#endif
                    // ---- every (direction, transverse mode, line) at once, one lane or a pair of lanes each
                    {
                        LaneLine o = my;
                        for (int sl_ = tid;;) {                  // one call site: slot tid from the registers, any further slot decoded on the way
                            if (o.ok) serial_line_hi<NB>(o.x, o.o1, o.o2, o.L, hPC, o.y, o.d0, o.dm, o.Ta, o.c, o.cnt, o.sl, o.tw, o.top);
                            sl_ += nt;
                            if (sl_ >= aSlots) break;
                            o = lane_line(sl_);
                        }
                    }
                    __syncthreads();
#ifdef NF_STAMPS
                    long long ts1 = (long long)__builtin_readcyclecounter();
#endif
                    double qv[KD], dot = 0.0;
#pragma unroll
                    for (int k = 0; k < KD; ++k) {
                        const int j = tid + k * 512; const bool in = j < hNPp;
                        const int jj = in ? j : 0;
                        double q_ = cv[k] * pv[k] + hc[0][jj];
                        if (A.dim >= 2) q_ += hc[1][jj];
                        if (A.dim == 3) q_ += hc[2][jj];
                        qv[k] = in ? q_ : 0.0; dot += pv[k] * qv[k];
                    }
#ifdef NF_STAMPS
                    long long ts2 = (long long)__builtin_readcyclecounter();
#endif
                    const double pq = block_total_1b(dot, sred, 0);   // src/solvers.cpp:602-606
#ifdef NF_STAMPS
                    long long ts3 = (long long)__builtin_readcyclecounter();
#endif
                    if (fabs(pq) < 1e-30) break;
                    const double alpha = rr / pq;
                    s = 0.0;
#pragma unroll
                    for (int k = 0; k < KD; ++k) { rv[k] = rv[k] - alpha * qv[k]; s += rv[k] * rv[k]; }
                    const double rr_new = block_total_1b(s, sred, 1);   // :613-631
                    ++its;
                    const bool conv = rr_new < tol_sq;
                    const double beta = rr_new / rr; rr = rr_new;
#pragma unroll
                    for (int k = 0; k < KD; ++k) {                // :609, :630
                        xv[k] = fma(alpha, pv[k], xv[k]);
                        pv[k] = fma(beta, pv[k], rv[k]);
                        if (tid + k * 512 < hNPp) hp[tid + k * 512] = pv[k];
                    }
                    __syncthreads();
#ifdef NF_STAMPS
                    if (tid == 0 && A.hist) { long long ts4 = (long long)__builtin_readcyclecounter(); long long *acc = (long long *)(A.hist + 3 * A.max_outer);
                                              acc[0] += ts1 - ts0; acc[1] += ts2 - ts1; acc[2] += ts3 - ts2; acc[3] += ts4 - ts3; acc[4] += 1; }
#endif
                    if (conv) break;
                }
#pragma unroll
                for (int k = 0; k < KD; ++k) if (gj[k] >= 0) graw[gj[k]] = xv[k];
                if (tid == 0) A.hist_cg[it * ng + g] = its;
                cg_total += its;
                __syncthreads();
                continue;
            }
            if constexpr (SERIAL) {
                double *const graw = A.raw + (long)g * N;
                double rv[KC], xv[KC], cv[KC], pv[KC];
                // this group's factors into the directions' blocks, first pivots, C diagonal into registers
#pragma unroll
                for (int d = 0; d < 3; ++d) if (d < A.dim) {
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
                        const int ip = tid + k * 512;
                        lb[d][ip] = gi[k] >= 0 ? A.L[d][g * N + gi[k]] : 0.0;
                        lb[d][PITCH + ip] = gi[k] >= 0 ? A.DR[d][g * N + gi[k]] : 0.0;
                    }
                    for (int i = tid; i < (int)A.nlines[d]; i += nt) ((lds_f64 *)lD[d])[i] = A.D0[d][g * A.nlines[d] + i];
                }
                const int nx = A.G.nx, ny = A.G.ny;
                // two-sided directions: the odd lane of every pair rewrites the upper half of its line with the mirrored factors
                __syncthreads();
                for (int sl_ = tid; sl_ < aSlots; sl_ += nt) {
                    const int d = sl_ >= aS0.c ? 2 : sl_ >= aS0.b ? 1 : 0;
                    const int rem = sl_ - (aS0[d]);
                    const int twd = aTw[d], nl = aNl[d];
                    const int l = rem >> 1;
                    if (twd && (rem & 1) && l < nl) {
                        const int base = d == 0 ? l * nxp : d == 1 ? (l / nx) * nxp * ny + l % nx : (l / nx) * nxp + l % nx;
                        const int sl = d == 0 ? 1 : d == 1 ? nxp : nxp * ny, n = d == 0 ? nx : d == 1 ? ny : A.G.nz;
                        lds_f64 *const Lb = (d == 0 ? lb[0] : d == 1 ? lb[1] : lb[2]) + base;
                        const lds_f64 *const D0d = d == 0 ? lD[0] : d == 1 ? lD[1] : lD[2];
                        double dm;
                        const double first = serial_twist_factors(Lb, PITCH, D0d[l], n, n / 2, sl, dm);
                        (d == 0 ? lDm[0] : d == 1 ? lDm[1] : lDm[2])[l] = dm;
                        (d == 0 ? lDr[0] : d == 1 ? lDr[1] : lDr[2])[l] = first;
                    }
                }
                // rhs = chi_g tf / k + scatter (Gauss-Seidel) (:1716-1726); CG start x = 0, r = p = rhs (src/solvers.cpp:583-592)
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    double v = 0.0; cv[k] = 0.0;
                    if (gi[k] >= 0) {
                        const int i = gi[k];
                        v = inv_k * (A.Chi[g * N + i] * A.tf[i]);
                        for (int gp = 0; gp < ng; ++gp) {
                            const double *M = A.Ms[g * ng + gp];
                            if (gp == g || !M) continue;
                            v += M[i] * (gp < g ? A.raw : A.phi)[gp * N + i];
                        }
                        cv[k] = A.Cd0[g * N + i];
                    }
                    rv[k] = v; pv[k] = v; xv[k] = 0.0; lp[tid + k * 512] = v; s += v * v;
                }
                double rr = block_total(s, sred);
                const double rhs_norm = sqrt(rr), tol_sq = A.cg_tol * A.cg_tol * rhs_norm * rhs_norm;
                int its = 0;
                // which line (half) a lane slot sweeps; slot `tid` is decoded once per group, not once per iteration
                struct LaneLine { bool ok, tw, top; int cnt, base, sl; double d0, dm, Ta; lds_f64 *blk; };
                auto lane_line = [&](int sl_) -> LaneLine {
                    LaneLine o; o.ok = false; o.tw = o.top = false; o.cnt = o.base = o.sl = 0; o.d0 = o.dm = o.Ta = 0.0; o.blk = lb[0];
                    if (sl_ >= aSlots) return o;
                    const int d = sl_ >= aS0.c ? 2 : sl_ >= aS0.b ? 1 : 0;
                    const int rem = sl_ - (aS0[d]);
                    const int twd = aTw[d], nl = aNl[d];
                    const int l = twd ? rem >> 1 : rem;
                    if (l >= nl) return o;
                    o.ok = true; o.tw = twd != 0; o.top = !twd || !(rem & 1);
                    const int base0 = d == 0 ? l * nxp : d == 1 ? (l / nx) * nxp * ny + l % nx : (l / nx) * nxp + l % nx;
                    const int sl0 = d == 0 ? 1 : d == 1 ? nxp : nxp * ny, n = d == 0 ? nx : d == 1 ? ny : A.G.nz;
                    o.cnt = !twd ? n : o.top ? n / 2 : n - n / 2;
                    o.base = o.top ? base0 : base0 + (n - 1) * sl0; o.sl = o.top ? sl0 : -sl0;
                    o.Ta = aTa[d];
                    o.blk = d == 0 ? lb[0] : d == 1 ? lb[1] : lb[2];
                    o.d0 = o.top ? (d == 0 ? lD[0] : d == 1 ? lD[1] : lD[2])[l] : (d == 0 ? lDr[0] : d == 1 ? lDr[1] : lDr[2])[l];
                    o.dm = twd ? (d == 0 ? lDm[0] : d == 1 ? lDm[1] : lDm[2])[l] : 0.0;
                    return o;
                };
                const LaneLine my = lane_line(tid);
                while (its < A.cg_max) {
#ifdef NF_STAMPS
                    long long ts0 = (long long)__builtin_readcyclecounter();
#endif
                    // ---- every line of every direction at once, one lane (or a pair of lanes) each: X p, Y p, Z p into the directions' blocks
                    {
                        LaneLine o = my;
                        for (int sl_ = tid;;) {                  // one call site: slot tid from the registers, any further slot decoded on the way
                            if (o.ok) serial_line_rt0<PITCH>(lp, o.blk, o.d0, o.dm, o.Ta, o.cnt, o.base, o.sl, o.tw, o.top);
                            sl_ += nt;
                            if (sl_ >= aSlots) break;
                            o = lane_line(sl_);
                        }
                    }
                    __syncthreads();
#ifdef NF_STAMPS
                    long long ts1 = (long long)__builtin_readcyclecounter();
#endif
                    // ---- own cells: q = C p + X p + Y p + Z p and p.q
                    double qv[KC], dot = 0.0;
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
                        const int ip = tid + k * 512;
                        double q_ = cv[k] * pv[k] + lb[0][2 * PITCH + ip];
                        if (A.dim >= 2) q_ += lb[1][2 * PITCH + ip];
                        if (A.dim == 3) q_ += lb[2][2 * PITCH + ip];
                        qv[k] = q_; dot += pv[k] * q_;
                    }
#ifdef NF_STAMPS
                    long long ts2 = (long long)__builtin_readcyclecounter();
#endif
                    const double pq = block_total_1b(dot, sred, 0);   // src/solvers.cpp:602-606
#ifdef NF_STAMPS
                    long long ts3 = (long long)__builtin_readcyclecounter();
#endif
                    if (fabs(pq) < 1e-30) break;
                    const double alpha = rr / pq;
                    s = 0.0;
#pragma unroll
                    for (int k = 0; k < KC; ++k) { rv[k] = rv[k] - alpha * qv[k]; s += rv[k] * rv[k]; }
                    const double rr_new = block_total_1b(s, sred, 1);   // :613-631
                    ++its;
                    const bool conv = rr_new < tol_sq;
                    const double beta = rr_new / rr; rr = rr_new;
#pragma unroll
                    for (int k = 0; k < KC; ++k) {                // :609, :630
                        xv[k] = fma(alpha, pv[k], xv[k]);
                        pv[k] = fma(beta, pv[k], rv[k]);
                        lp[tid + k * 512] = pv[k];
                    }
                    __syncthreads();
#ifdef NF_STAMPS
                    if (tid == 0 && A.hist) { long long ts4 = (long long)__builtin_readcyclecounter(); long long *acc = (long long *)(A.hist + 3 * A.max_outer);
                                              acc[0] += ts1 - ts0; acc[1] += ts2 - ts1; acc[2] += ts3 - ts2; acc[3] += ts4 - ts3; acc[4] += 1; }
#endif
                    if (conv) break;
                }
#pragma unroll
                for (int k = 0; k < KC; ++k) if (gi[k] >= 0) graw[gi[k]] = xv[k];
                if (tid == 0) A.hist_cg[it * ng + g] = its;
                cg_total += its;
                __syncthreads();
                continue;
            }
            double *const graw = A.raw + (long)g * NP;
            double *const xsol = vx ? vx : graw;
            // this group's line factors and C diagonal into LDS (when planned)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (fL[d]) for (long i = tid; i < N; i += nt) fL[d][i] = A.L[d][g * N + i];
                if (fR[d]) for (long i = tid; i < N; i += nt) fR[d][i] = A.DR[d][g * N + i];
            }
            if (fC) for (long i = tid; i < NP; i += nt) fC[i] = A.Cd0[g * NP + i];
            // rhs = chi_g tf / k + scatter (Gauss-Seidel) (:1716-1726); CG start x = 0, r = p = rhs (src/solvers.cpp:583-592)
            s = 0.0;
            for (long i = tid; i < NP; i += nt) {
                double v;
                if (NP == N) v = inv_k * (A.Chi[g * N + i] * A.tf[i]);
                else { const double cv = A.Chi[g * N + i % N] * inv_k; v = fabs(cv) < 1e-14 ? 0.0 : cv * A.tf[i]; }
                for (int gp = 0; gp < ng; ++gp) {
                    const double *M = A.Ms[g * ng + gp];
                    if (gp == g || !M) continue;
                    v += M[i] * (gp < g ? A.raw : A.phi)[gp * NP + i];
                }
                xsol[i] = 0.0; wr[i] = v; wp[i] = v; s += v * v;
            }
            double rr = block_total(s, sred);
            const double rhs_norm = sqrt(rr), tol_sq = A.cg_tol * A.cg_tol * rhs_norm * rhs_norm;
            int its = 0, pend = 0; double alpha = 0.0, beta = 0.0;
            const CgFuse fz = { wp, wr, xsol, nullptr };
            ModeArgs mad[3];
            const double *dL[3], *dR[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                mad[d] = A.ma[d]; mad[d].D += g * N;
                for (int q = 0; q <= NB; ++q) {
                    const long off = A.ma[d].x[q] - A.p;         // offset of this moment inside a flux vector
                    mad[d].x[q] = wp + off; mad[d].y[q] = wq + off;
                    mad[d].Cd[q] = fC ? fC + off : A.Cd0 + g * NP + off;
                }
                dL[d] = fL[d] ? fL[d] : A.L[d] + g * N; dR[d] = fR[d] ? fR[d] : A.DR[d] + g * N;
            }
            while (its < A.cg_max) {
                const bool fuse = its > 0;
                double dot = 0.0;
#ifdef NF_STAMPS
                long long ts0 = (long long)__builtin_readcyclecounter();
#endif
                // ---- x lines: q = C p + X p, carrying the deferred x_sol += alpha p, p = r + beta p of the previous iteration
                const int ntask = A.ntask_x * A.nmodes;
                for (int gt0 = 0; gt0 < ntask; gt0 += nw) {
                    const int gt = gt0 + wave;
                    const bool active = gt < ntask;
                    const int mode = active ? gt / A.ntask_x : 0;
                    const ModeArgs ma = select_mode(mad[0], A.mt[0], mode, NB + 1);
                    const double dx = schur_x_task<2, 1, VEC, NB, NoMid, true>(ma, A.G, dL[0], dR[0], A.D0[0] + g * A.nlines[0], A.G.nx, A.G.ny,
                                                                  A.nlines[0], A.lpl_log2, 1, gt % A.ntask_x, tid & 63, active, fuse, alpha, beta, fz);
                    if (A.dim == 1) dot += dx;
                }
                __syncthreads();
#ifdef NF_STAMPS
                long long ts1 = (long long)__builtin_readcyclecounter();
#endif
                // ---- y, then z lines: accumulate into q; the last direction also gives p.q
                if (A.dim >= 2) { const double ds = resident_s_pass<SEG, 1, NB>(A, 0, mad[1], dL[1], dR[1], g, sm, sa0, fz); if (A.dim == 2) dot += ds; }
                if (A.dim == 3) dot += resident_s_pass<SEG, 2, NB>(A, 1, mad[2], dL[2], dR[2], g, sm, sa0, fz);
#ifdef NF_STAMPS
                long long ts2 = (long long)__builtin_readcyclecounter();
#endif
                const double pq = block_total(dot, sred);       // src/solvers.cpp:602-606
#ifdef NF_STAMPS
                long long ts3 = (long long)__builtin_readcyclecounter();
#endif
                pend = 0;
                if (fabs(pq) < 1e-30) break;
                alpha = rr / pq;
                s = 0.0;
                for (long i = tid; i < NP; i += nt) { const double rn = wr[i] - alpha * wq[i]; wr[i] = rn; s += rn * rn; }
                const double rr_new = block_total(s, sred);     // :613-631
#ifdef NF_STAMPS
                if (tid == 0 && A.hist) { long long ts4 = (long long)__builtin_readcyclecounter(); long long *acc = (long long *)(A.hist + 3 * A.max_outer);
                                          acc[0] += ts1 - ts0; acc[1] += ts2 - ts1; acc[2] += ts3 - ts2; acc[3] += ts4 - ts3; acc[4] += 1; }
#endif
                ++its; pend = 1;
                if (rr_new < tol_sq) { rr = rr_new; break; }
                beta = rr_new / rr; rr = rr_new;
            }
            // the last iteration's x_sol update; the group's solution goes (back) to global memory
            if (pend) for (long i = tid; i < NP; i += nt) graw[i] = fma(alpha, wp[i], xsol[i]);
            else if (vx) for (long i = tid; i < NP; i += nt) graw[i] = xsol[i];
            if (tid == 0) A.hist_cg[it * ng + g] = its;
            cg_total += its;
            __syncthreads();
        }
        // prod_new, norms (:1766-1779)
        double sp = 0.0, sn = 0.0, sd = 0.0;
        for (long i = tid; i < NT; i += nt) { const double v = A.raw[i], d = v - A.phi[i]; sp += A.Mf[i] * v; sn += v * v; sd += d * d; }
        const double prod_new = block_total(sp, sred), nsq = block_total(sn, sred), dsq = block_total(sd, sred);
        const OuterStep os = outer_step(keff, it, prod_old, prod_new, nsq, dsq);
        keff = os.keff;
        if (tid == 0) { A.hist[it] = keff; A.hist[A.max_outer + it] = os.dk; A.hist[2 * A.max_outer + it] = os.dphi; }
        n_outer = it + 1;
        if (!os.finite) { status = 2; break; }
        // normalise + Chebyshev (:1780-1788, src/solvers.cpp:720-756)
        const ChebStep cs = cheb_next(cheb_it, A.cheb, it >= 2);
        for (long i = tid; i < NT; i += nt) A.phi[i] = cheb_update(A.raw[i], os.do_norm, os.norm, cs, pa, pb, i);
        if (cs.mode == 3) { double *t = pa; pa = pb; pb = t; }
        __syncthreads();
        if (outer_converged(os.dk, os.dphi, A.tol_keff, A.tol_flux)) break;   // :1799-1802
    }
    if (tid == 0) { A.out->keff = keff; A.out->n_outer = n_outer; A.out->status = status; A.out->cg_total = cg_total; }
}
template <bool VEC, int NB, int PITCH = 0>
__global__ __launch_bounds__(512) void k_resident_keff(ResidentArgs A) { resident_keff_body<VEC, NB, PITCH>(A); }
// N independent meshes in one launch, workgroup b solves args[b] (nf_solve_keff_batch).  No workgroup waits for another,
// so a grid larger than the chip simply runs in turns.  args[b] has to behave like the kernel argument of the entry above: a uniform
// address, scalar loads where a member is used, known not to change under the body's barriers and stores, never copied to registers or
// scratch, and the pointers in it known to be global ones (SGPR base + lane offset, not a 64-bit flat address per lane).  A by-value
// kernel argument is all that because it lies in the constant address space; so the array is declared there.  (Reading a plain global
// pointer through a constant-address-space cast gives the scalar loads but leaves the pointers flat: +16 VGPRs and spills at RT1 / RT2.)
typedef __attribute__((address_space(4))) const ResidentArgs ResidentArgsConst;
template <bool VEC, int NB, int PITCH = 0>
__global__ __launch_bounds__(512) void k_resident_keff_batch(ResidentArgsConst *args, int n)
{
    const int b = blockIdx.x;
    if (b >= n) return;
    resident_keff_body<VEC, NB, PITCH>(*(const ResidentArgs *)(args + b));
}

// ---------------------------------------------------------------------------------------------
// Explicit-S branch of the Schur solver (src/solvers.cpp:114-124, 259-509: direct solver types, a never-pushed solver type,
// n_phi < 200): S is formed column by column with the matrix-free apply (S e_j), inverted once per BuildMatrices, and a
// group solve is one dense matrix-vector product.  Column-major n x n.
__global__ void k_unit_vector(double *__restrict__ v, long n, long j)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) v[i] = i == j ? 1.0 : 0.0;
}
// one step of the in-place-style Gauss-Jordan inversion (S is SPD: no pivoting), written out of place so that every entry reads
// the step's pivot row and column as they were: Mo = step_k(M)
__global__ void k_gj_step(const double *__restrict__ M, double *__restrict__ Mo, int n, int k)
{
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)n * n) return;
    const int i = (int)(idx % n), j = (int)(idx / n);
    const double p = M[(long)k * n + k], rkj = M[(long)j * n + k], fik = M[(long)k * n + i];
    double out;
    if (i == k && j == k) out = 1.0 / p;
    else if (i == k) out = rkj / p;
    else if (j == k) out = -fik / p;
    else out = M[idx] - fik * (rkj / p);
    Mo[idx] = out;
}
// y = Sinv x: one thread per row, consecutive threads read consecutive rows of a column (coalesced)
__global__ void k_dense_matvec(const double *__restrict__ Sinv, const double *__restrict__ x, double *__restrict__ y, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += Sinv[(long)j * n + i] * x[j];
    y[i] = s;
}

// adjoint helpers: sum over groups, weighted dot product, scaling
__global__ void k_sum_groups(const double *__restrict__ a, double *__restrict__ out, long n, int ng)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) { double v = 0.0; for (int g = 0; g < ng; ++g) v += a[g * n + i]; out[i] = v; }
}
// partial sums of sum_g sum_i a[g][i] b[g][i] m[i]   (bi-orthonormalisation <phi, phi+>, :2020-2066)
__global__ __launch_bounds__(256) void k_dot3(const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ m,
                                              long n, int ng, double *__restrict__ partials)
{
    __shared__ double sred[4];
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n * ng; i += gridDim.x * 256L) s += a[i] * b[i] * m[i % n];
    s = block_sum(s, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
__global__ void k_scale(double *__restrict__ v, long n, double divisor)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) v[i] /= divisor;
}
__global__ void k_fill_const(double *__restrict__ v, long n, double c)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) v[i] = c;
}

// SolveCoarse: arithmetic volume-weighted block means (src/NeutFEM.cpp:2494-2556), one thread per coarse cell
__global__ void k_coarsen(const double *__restrict__ fine, double *__restrict__ coarse, const double *__restrict__ xb,
                          const double *__restrict__ yb, const double *__restrict__ zb, int dim, int nx, int ny, int nz,
                          int rx, int ry, int rz, int nfields)
{
    const int nxc = nx / rx, nyc = ny / ry, nzc = nz / rz;
    const long Nc = (long)nxc * nyc * nzc, Nf = (long)nx * ny * nz;
    const long ec = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (ec >= Nc) return;
    const int kx = (int)(ec % nxc), ky = (int)((ec / nxc) % nyc), kz = (int)(ec / ((long)nxc * nyc));
    for (int f = 0; f < nfields; ++f) {
        double vt = 0.0, s = 0.0;
        for (int sz = 0; sz < rz; ++sz) for (int sy = 0; sy < ry; ++sy) for (int sx = 0; sx < rx; ++sx) {
            const int ixf = kx * rx + sx, iyf = ky * ry + sy, izf = kz * rz + sz;
            double vol = xb[ixf + 1] - xb[ixf];
            if (dim >= 2) vol *= yb[iyf + 1] - yb[iyf];
            if (dim >= 3) vol *= zb[izf + 1] - zb[izf];
            vt += vol;
            s += vol * fine[f * Nf + ((long)izf * ny + iyf) * nx + ixf];
        }
        coarse[f * Nc + ec] = s / vt;
    }
}
// prolongation: piecewise-constant injection (src/NeutFEM.cpp:2585-2606)
// fine has gstride doubles per group (nloc*Nf, SoA): only the P0 moment is written, the rest is zeroed by the caller
__global__ void k_prolong(const double *__restrict__ coarse, double *__restrict__ fine, int nx, int ny, int nz, int rx,
                          int ry, int rz, int ng, long gstride)
{
    const long Nf = (long)nx * ny * nz;
    const int nxc = nx / rx, nyc = ny / ry; const long Nc = (long)nxc * nyc * (nz / rz);
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= Nf) return;
    const int ix = (int)(e % nx), iy = (int)((e / nx) % ny), iz = (int)(e / ((long)nx * ny));
    const long ec = ((long)(iz / rz) * nyc + iy / ry) * nxc + ix / rx;
    for (int g = 0; g < ng; ++g) fine[g * gstride + e] = coarse[g * Nc + ec];
}

// J reconstruction (src/solvers.cpp:227-228 full path: J = -A^-1 B^T phi ; src/NeutFEM.cpp:620-633 diagonal
// path: J_f = +(B^T phi)_f / A_ff).  One thread per (line, transverse mode), Thomas in place in the face array (run
// once, after convergence).  Face DOF (face, a) lives at face*nf + a; bubble (l, a) of cell e at e*ni + l + k*a behind the
// faces (src/FEM.cpp:264-334, 377-397).  jface / jbub point at this direction's face / bubble block; nfa = (k+1)^(dim-1).
__global__ void k_flux_to_J(Geom G, ModeArgs ma, int nb, int amode, int nfa, int ni, const double *__restrict__ D,
                            const double *__restrict__ L, const double *__restrict__ DR, const double *__restrict__ D0,
                            double *__restrict__ jface, double *__restrict__ jbub, long nlines, int diag,
                            const unsigned char *__restrict__ voidm = nullptr)
{
    const long line = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (line >= nlines) return;
    const int d = ma.dir;
    int n, ix = 0, iy = 0, iz = 0; long base, sl, fbase, fsl;
    const long nxy = (long)G.nx * G.ny;
    if (d == 0) { n = G.nx; iy = (int)(line % G.ny); iz = (int)(line / G.ny); base = line * G.nx; sl = 1; fbase = line * (G.nx + 1); fsl = 1; }
    else if (d == 1) { n = G.ny; ix = (int)(line % G.nx); iz = (int)(line / G.nx); base = iz * nxy + ix; sl = G.nx;
                       fbase = (long)iz * (G.ny + 1) * G.nx + ix; fsl = G.nx; }
    else { n = G.nz; ix = (int)(line % G.nx); iy = (int)(line / G.nx); base = line; sl = nxy; fbase = line; fsl = nxy; }
    int *ci = d == 0 ? &ix : d == 1 ? &iy : &iz;
#define JF(f) jface[(fbase + (long)(f) * fsl) * nfa + amode]
    if (!diag) {
        // xL / xR of a cell (ModeArgs), forward sweep, scaling, backward sweep; faces hold z, then u, then -u
        auto xlr = [&](int c, double &xl, double &xr) {
            const long a = base + (long)c * sl;
            double pl = 0.0, pr = 0.0;
            for (int l = 0; l < nb; ++l) { const double gx = ma.Gc[l] * ma.x[l + 1][a]; pl += ma.eL[l] * gx; pr += ma.eR[l] * gx; }
            xl = ma.x[0][a] + pl; xr = ma.x[0][a] - pr;
        };
        double xl, xr; xlr(0, xl, xr);
        double z = -xl;
        JF(0) = z * D0[line];
        for (int c = 0; c < n; ++c) {
            double nxl = 0.0, nxr = 0.0;
            if (c + 1 < n) xlr(c + 1, nxl, nxr);
            z = (xr - nxl) - L[base + (long)c * sl] * z;
            JF(c + 1) = z * DR[base + (long)c * sl];
            xr = nxr;
        }
        double u = JF(n);
        for (int c = n - 1; c >= 0; --c) {
            const double uhi = u;
            u = JF(c) - L[base + (long)c * sl] * u;
            JF(c + 1) = -uhi;
            // bubbles of cell c: v_l = G_l x_{l+1} iM_l / c_e - (eL_l u_c + eR_l u_{c+1}); inactive bubbles (l >= nb) have t_b = 0
            if (ni > 0) {
                *ci = c;
                const long a = base + (long)c * sl;
                const double ic = D[a] / geom_factor(G, d, ix, iy, iz);
                for (int l = 0; l < G.k; ++l) {
                    const double tb = l < nb ? ma.Gc[l] * ma.x[l + 1][a] * ma.iM[l] * ic : 0.0;
                    const double v = tb - (ma.eL[l] * u + ma.eR[l] * uhi);
                    jbub[a * ni + l + G.k * amode] = voidm && voidm[a] ? 0.0 : -v;   // nf_set_void: identity rows with a zero load
                }
            }
        }
        JF(0) = -u;
    } else {
        double a2p = 0.0, a1, xp = 0.0, Dp = 0.0;
        for (int f = 0; f <= n; ++f) {
            double a2 = 0.0, xc = 0.0, Dc = 0.0;
            if (f < n) { *ci = f; Dc = D[base + (long)f * sl]; cell_a(G, d, ix, iy, iz, Dc, a2, a1); xc = ma.x[0][base + (long)f * sl]; }
            double Aff = a2p + a2;
            if (f == 0 && G.dir_lo[d]) { *ci = 0; Aff += dirichlet_term(G, d, ix, iy, iz, Dc); }
            if (f == n && G.dir_hi[d]) { *ci = n - 1; Aff += dirichlet_term(G, d, ix, iy, iz, Dp); }
            const double tt = xp - xc;                           // (B^T phi)_f / A_ff = T0 (..) / (T0 A_unit)
            JF(f) = fabs(G.T0 * Aff) < 1e-14 ? 0.0 : tt / Aff;
            a2p = a2; xp = xc; Dp = Dc;
        }
    }
#undef JF
}

// Diagonal-path currents of the z faces of a slab (src/NeutFEM.cpp:620-633: J_f = (B^T phi)_f / A_ff): the interface faces take the
// neighbour's edge-cell value and a2 (one plane each, exchanged by the caller); both slabs of an interface report the same number.
__global__ void k_diag_Jz_slab(Geom G, const double *__restrict__ D, const double *__restrict__ x, double *__restrict__ jz, long nlines,
                               int if_lo, int if_hi, const double *__restrict__ nb_x_lo, const double *__restrict__ nb_a2_lo,
                               const double *__restrict__ nb_x_hi, const double *__restrict__ nb_a2_hi)
{
    const long line = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (line >= nlines) return;
    const int ix = (int)(line % G.nx), iy = (int)(line / G.nx), n = G.nz;
    const long nxy = (long)G.nx * G.ny;
    double a2p = if_lo ? nb_a2_lo[line] : 0.0, xp = if_lo ? nb_x_lo[line] : 0.0, Dp = 0.0, a1;
    for (int f = 0; f <= n; ++f) {
        double a2 = 0.0, xc = 0.0, Dc = 0.0;
        if (f < n) { Dc = D[line + (long)f * nxy]; cell_a(G, 2, ix, iy, f, Dc, a2, a1); xc = x[line + (long)f * nxy]; }
        else if (if_hi) { a2 = nb_a2_hi[line]; xc = nb_x_hi[line]; }
        double Aff = a2p + a2;
        if (f == 0 && G.dir_lo[2]) Aff += dirichlet_term(G, 2, ix, iy, 0, Dc);
        if (f == n && G.dir_hi[2]) Aff += dirichlet_term(G, 2, ix, iy, n - 1, Dp);
        const double tt = xp - xc;
        jz[(long)f * nxy + line] = fabs(G.T0 * Aff) < 1e-14 ? 0.0 : tt / Aff;
        a2p = a2; xp = xc; Dp = Dc;
    }
}

// ---------------------------------------------------------------------------------------------
// CMFD acceleration (src/NeutFEM.cpp:662-1017).  A 7-point finite-volume operator per group on the cell grid,
//   M = diag(C_00 + sum_faces Deff A_face) - offdiag(Deff A_face),  Deff = D~ + D^,
// solved with Eigen's diagonally preconditioned CG (tolerance 1e-8 on |r|/|b|, at most 100 iterations, x0 = 0).  Face
// coefficients are stored per direction with the reference's face numbering (x: iz*ny*(nx+1) + iy*(nx+1) + ix, ...).
struct CmfdFaces { const double *Dt[3]; const double *Dh[3]; };
struct CmfdScalars { double absNew, alpha, beta, thr; int done, its; };

__device__ __forceinline__ double cmfd_face_area(const Geom &G, int d, int ix, int iy, int iz)
{
    return d == 0 ? G.hy[iy] * G.hz[iz] : d == 1 ? G.hx[ix] * G.hz[iz] : G.hx[ix] * G.hy[iy];
}
__device__ __forceinline__ long cmfd_face(const Geom &G, int d, int ix, int iy, int iz)
{
    if (d == 0) return ((long)iz * G.ny + iy) * (G.nx + 1) + ix;
    if (d == 1) return ((long)iz * (G.ny + 1) + iy) * G.nx + ix;
    return ((long)iz * G.ny + iy) * G.nx + ix;
}
// ComputeDtildeCoefficients (:723-821): harmonic mean inside, 2D/h on the boundary.  One thread per face of direction d.
__global__ void k_cmfd_dtilde(Geom G, int d, const double *__restrict__ D, double *__restrict__ Dt, long nfaces)
{
    const long f = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (f >= nfaces) return;
    const int n0 = d == 0 ? G.nx + 1 : G.nx, n1 = d == 1 ? G.ny + 1 : G.ny;
    int c[3] = { (int)(f % n0), (int)((f / n0) % n1), (int)(f / ((long)n0 * n1)) };
    const int nd = d == 0 ? G.nx : d == 1 ? G.ny : G.nz;
    const double *h = d == 0 ? G.hx : d == 1 ? G.hy : G.hz;
    const int cd = c[d];
    const long st = d == 0 ? 1 : d == 1 ? G.nx : (long)G.nx * G.ny;
    c[d] = cd == 0 ? 0 : cd - 1;                                  // lower (or only) neighbour
    const long eL = ((long)c[2] * G.ny + c[1]) * G.nx + c[0];
    double v;
    if (cd == 0 || cd == nd) v = 2.0 * D[eL] / h[c[d]];
    else { const double DL = D[eL], DR = D[eL + st], dL = h[cd - 1], dR = h[cd]; v = 2.0 * DL * DR / (DL * dR + DR * dL); }
    Dt[f] = v;
}
// UpdateDhatCoefficients (:823-869): x faces only; Jx holds the mode-0 face current at stride nfa.
__global__ void k_cmfd_dhat(Geom G, const double *__restrict__ phi, const double *__restrict__ Jx, int nfa,
                            const double *__restrict__ Dt, double *__restrict__ Dh, long nfaces)
{
    const long f = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (f >= nfaces) return;
    const int ix = (int)(f % (G.nx + 1)); const long line = f / (G.nx + 1);
    const long eR = line * G.nx + ix, eL = eR - 1;
    const double pd = ix == 0 ? -phi[eR] : ix == G.nx ? phi[eL] : phi[eL] - phi[eR];
    Dh[f] = fabs(pd) > 1e-14 ? Jx[f * nfa] / pd - Dt[f] : 0.0;
}
__device__ __forceinline__ void cmfd_cell(const Geom &G, long e, int &ix, int &iy, int &iz)
{
    ix = (int)(e % G.nx); iy = (int)((e / G.nx) % G.ny); iz = (int)(e / ((long)G.nx * G.ny));
}
// diag, rhs = chi tf / k, x = 0, r = rhs, p = z = r / diag ; partials: [0] |rhs|^2, [1] r.z
__global__ __launch_bounds__(256) void k_cmfd_setup(Geom G, CmfdFaces F, const double *__restrict__ C00, const double *__restrict__ chi,
                                                    const double *__restrict__ tf, double inv_k, double *__restrict__ diag,
                                                    double *__restrict__ x, double *__restrict__ r, double *__restrict__ pp,
                                                    long N, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    double s0 = 0.0, s1 = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        int c[3]; cmfd_cell(G, e, c[0], c[1], c[2]);
        double dg = C00[e];
        for (int d = 0; d < G.dim; ++d) {
            const double A = cmfd_face_area(G, d, c[0], c[1], c[2]);
            const long fl = cmfd_face(G, d, c[0], c[1], c[2]);
            c[d] += 1; const long fu = cmfd_face(G, d, c[0], c[1], c[2]); c[d] -= 1;
            dg += ((F.Dt[d][fl] + F.Dh[d][fl]) + (F.Dt[d][fu] + F.Dh[d][fu])) * A;
        }
        const double b = chi[e] * tf[e] * inv_k;
        const double z = (dg != 0.0 ? 1.0 / dg : 1.0) * b;             // DiagonalPreconditioner stores 1/diag
        diag[e] = dg; x[e] = 0.0; r[e] = b; pp[e] = z;
        s0 += b * b; s1 += b * z;
    }
    s0 = block_sum(s0, sred); s1 = block_sum(s1, sred);
    if (threadIdx.x == 0) { partials[blockIdx.x] = s0; partials[stride + blockIdx.x] = s1; }
}
// q = M p ; partial p.q
// nb_lo / nb_hi (slabs): the neighbouring slab's edge plane of p across the interface below / above, else nullptr
__global__ __launch_bounds__(256) void k_cmfd_matvec(Geom G, CmfdFaces F, const double *__restrict__ diag, const double *__restrict__ pp,
                                                     double *__restrict__ q, long N, const CmfdScalars *__restrict__ sc,
                                                     double *__restrict__ partials, const double *__restrict__ nb_lo, const double *__restrict__ nb_hi)
{
    __shared__ double sred[4];
    if (sc->done) return;
    const long nxy = (long)G.nx * G.ny;
    double s0 = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        int c[3]; cmfd_cell(G, e, c[0], c[1], c[2]);
        const double pe = pp[e];
        double s = diag[e] * pe;
        for (int d = 0; d < G.dim; ++d) {
            const int cd = c[d], nd = d == 0 ? G.nx : d == 1 ? G.ny : G.nz;
            const long st = d == 0 ? 1 : d == 1 ? G.nx : nxy;
            const double A = cmfd_face_area(G, d, c[0], c[1], c[2]);
            const long fl = cmfd_face(G, d, c[0], c[1], c[2]);
            c[d] += 1; const long fu = cmfd_face(G, d, c[0], c[1], c[2]); c[d] -= 1;
            if (cd > 0) s -= (F.Dt[d][fl] + F.Dh[d][fl]) * A * pp[e - st];
            else if (d == 2 && nb_lo) s -= (F.Dt[d][fl] + F.Dh[d][fl]) * A * nb_lo[e % nxy];
            if (cd < nd - 1) s -= (F.Dt[d][fu] + F.Dh[d][fu]) * A * pp[e + st];
            else if (d == 2 && nb_hi) s -= (F.Dt[d][fu] + F.Dh[d][fu]) * A * nb_hi[e % nxy];
        }
        q[e] = s; s0 += pe * s;
    }
    s0 = block_sum(s0, sred);
    if (threadIdx.x == 0) partials[blockIdx.x] = s0;
}
// x += alpha p ; r -= alpha q ; z = r / diag ; partials: [0] |r|^2, [1] r.z
__global__ __launch_bounds__(256) void k_cmfd_update(const double *__restrict__ diag, const double *__restrict__ pp, const double *__restrict__ q,
                                                     double *__restrict__ x, double *__restrict__ r, double *__restrict__ z, long N,
                                                     const CmfdScalars *__restrict__ sc, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    if (sc->done) return;
    const double alpha = sc->alpha;
    double s0 = 0.0, s1 = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        x[e] += alpha * pp[e];
        const double re = r[e] - alpha * q[e];
        const double dg = diag[e], ze = (dg != 0.0 ? 1.0 / dg : 1.0) * re;
        r[e] = re; z[e] = ze;
        s0 += re * re; s1 += re * ze;
    }
    s0 = block_sum(s0, sred); s1 = block_sum(s1, sred);
    if (threadIdx.x == 0) { partials[blockIdx.x] = s0; partials[stride + blockIdx.x] = s1; }
}
__global__ void k_cmfd_pupdate(const double *__restrict__ z, double *__restrict__ pp, long N, const CmfdScalars *__restrict__ sc)
{
    if (sc->done) return;
    const double beta = sc->beta;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) pp[e] = z[e] + beta * pp[e];
}
// Eigen's conjugate_gradient() scalar logic.  op 0: after setup (rhs2, r.z) ; op 1: after matvec (p.q) ; op 2: after update (|r|^2, r.z)
__device__ __forceinline__ void cmfd_logic(int op, const double *tot, CmfdScalars *sc)
{
    if (op == 0) {
        sc->its = 0; sc->alpha = sc->beta = 0.0;
        const double rhs2 = tot[0];
        sc->thr = fmax(1e-8 * 1e-8 * rhs2, 2.2250738585072014e-308);
        sc->absNew = tot[1];
        sc->done = (rhs2 == 0.0 || rhs2 < sc->thr) ? 1 : 0;
    } else if (op == 1) {
        sc->alpha = sc->absNew / tot[0];
    } else {
        sc->its += 1;
        if (tot[0] < sc->thr) { sc->done = 1; return; }
        sc->beta = tot[1] / sc->absNew;
        sc->absNew = tot[1];
        if (sc->its >= 100) sc->done = 1;
    }
}
// second reduction stage + the scalar logic.  One block of 256 threads.
__global__ __launch_bounds__(256) void k_cmfd_logic(int op, const double *__restrict__ partials, int cnt, long stride,
                                                    CmfdScalars *__restrict__ sc)
{
    __shared__ double sred[4];
    if (op != 0 && sc->done) return;
    double tot[2] = { 0.0, 0.0 };
    const int nq = op == 1 ? 1 : 2;
    for (int q = 0; q < nq; ++q) {
        double s = 0.0;
        for (int i = threadIdx.x; i < cnt; i += 256) s += partials[q * stride + i];
        tot[q] = block_sum(s, sred);
    }
    if (threadIdx.x != 0) return;
    cmfd_logic(op, tot, sc);
}
// slab teams: the totals come from k_finalize (reduce_only) + the all-reduce over ranks
__global__ void k_cmfd_logic_tot(int op, const double *__restrict__ red, CmfdScalars *__restrict__ sc)
{
    if (op != 0 && sc->done) return;
    double tot[2] = { red[0], op == 1 ? 0.0 : red[1] };
    cmfd_logic(op, tot, sc);
}
// D-tilde of the interface z faces of a slab (ComputeDtildeCoefficients interior formula, :760-790): the cell on the other side belongs
// to the neighbouring slab (its D and cell height arrive as planes).  Both slabs evaluate 2 DL DR / (DL dR + DR dL) with the same operands.
__global__ void k_cmfd_dtilde_iface(const double *__restrict__ D_own, const double *__restrict__ D_nb, const double *__restrict__ h_nb, double h_own,
                                    double *__restrict__ Dt_plane, long nlines, int own_is_upper)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= nlines) return;
    const double DL = own_is_upper ? D_nb[i] : D_own[i], DR = own_is_upper ? D_own[i] : D_nb[i];
    const double dL = own_is_upper ? h_nb[i] : h_own, dR = own_is_upper ? h_own : h_nb[i];
    Dt_plane[i] = 2.0 * DL * DR / (DL * dR + DR * dL);
}
// ratio clamp + relaxation (:994-1014); the correction multiplies every moment of the cell
__global__ void k_cmfd_correct(const double *__restrict__ x, double *__restrict__ phi, long N, int nloc, double omega)
{
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= N) return;
    const double pc = phi[e];
    double ratio = 1.0;
    if (fabs(pc) > 1e-14) { ratio = x[e] / pc; ratio = fmax(0.5, fmin(2.0, ratio)); }
    const double corr = omega * ratio + (1.0 - omega) * 1.0;
    for (int l = 0; l < nloc; ++l) phi[l * N + e] *= corr;
}

// streaming copy (HBM microbenchmark for the roofline's "of measured copy" figure): 16 bytes per lane and access, U independent loads in
// flight per lane before the first store, every block walks contiguous chunks of U x 4 KiB (a wave instruction covers 1 KiB); the grid is a
// multiple of the CU count.  NT = non-temporal loads and stores as whole 16-byte accesses (round 3's NT variant split them into two 8-byte
// halves and never got past 4.8 TB/s).
template <bool NT, int U>
__global__ __launch_bounds__(256) void k_copy(const nf_d2 *__restrict__ src, nf_d2 *__restrict__ dst, long n2)
{
    const long chunk = 256L * U;
    for (long base = (long)blockIdx.x * chunk; base < n2; base += (long)gridDim.x * chunk) {
        nf_d2 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = base + u * 256L + threadIdx.x;
            if (i < n2) v[u] = NT ? __builtin_nontemporal_load(src + i) : src[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = base + u * 256L + threadIdx.x;
            if (i < n2) { if (NT) __builtin_nontemporal_store(v[u], dst + i); else dst[i] = v[u]; }
        }
    }
}

// input validation on the device (nf_upload_xs): bit `bit` of *flags is raised if the array holds a non-finite value, or
// (need_nonzero) an exact zero -- 1/D of such a cell would put inf into every line system it touches
__global__ void k_check_xs(const double *__restrict__ v, long n, int need_nonzero, int bit, int *__restrict__ flags)
{
    bool bad = false;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const double x = v[i];
        bad |= !isfinite(x) || (need_nonzero && x == 0.0);
    }
    if (bad) atomicOr(flags, 1 << bit);
}

// ---- sub-cell projection (nf_project_flux / nf_project_power) ------------------------------------------------------------
// mean of P_0..P_M over sub-interval s of r equal parts of [-1, 1], [al, be] = [(2s - r) / r, (2s + 2 - r) / r]:
// 1, (al + be) / 2, (al^2 + al be + be^2 - 1) / 2.  r = 1 gives exactly 1, 0, 0; the last sub-interval ends exactly at 1.
template <int M>
__device__ __forceinline__ void sub_means(int s, int r, double *A)
{
    A[0] = 1.0;
    if (M >= 1) {
        const double rr = (double)r, al = (double)(2 * s - r) / rr, be = (double)(2 * s + 2 - r) / rr;
        A[1] = 0.5 * (al + be);
        if (M >= 2) A[2] = 0.5 * (al * al + al * be + be * be - 1.0);
    }
}
// x contraction of one cell for two x sub-intervals: s[q] = sum_i c_ijk A_i, q = j + nj k (nj = M+1 from 2D on), one load per coefficient.
// c = one group's coefficients in the device layout [p*N + e], p = i + (M+1) j + (M+1)^2 k = i + (M+1) q.  A_0 = 1: the i = 0 term is c itself
template <int DIM, int M>
__device__ __forceinline__ void x_contract2(const double *__restrict__ c, long N, long e, const double *A0, const double *A1, double *s0, double *s1)
{
    constexpr int n1 = M + 1, nq = (DIM >= 2 ? n1 : 1) * (DIM == 3 ? n1 : 1);
#pragma unroll
    for (int q = 0; q < nq; ++q) {
        const double c0 = c[(long)(n1 * q) * N + e];
        double v0 = c0, v1 = c0;
#pragma unroll
        for (int i = 1; i <= M; ++i) { const double ci = c[(long)(i + n1 * q) * N + e]; v0 += ci * A0[i]; v1 += ci * A1[i]; }
        s0[q] = v0; s1[q] = v1;
    }
}
// the y / z means of sub-row (B, Cz): sum_{j,k} B_j C_k s[j + nj k], the (0, 0) term (weight 1) first
template <int DIM, int M>
__device__ __forceinline__ double yz_contract(const double *s, const double *B, const double *Cz)
{
    constexpr int nj = DIM >= 2 ? M + 1 : 1, nk = DIM == 3 ? M + 1 : 1;
    double v = s[0];                                             // refine 1 and P0 give DOF 0 exactly
#pragma unroll
    for (int kk = 0; kk < nk; ++kk)
#pragma unroll
        for (int j = 0; j < nj; ++j)
            if (j || kk) v += s[j + nj * kk] * ((DIM >= 2 ? B[j] : 1.0) * (DIM == 3 ? Cz[kk] : 1.0));
    return v;
}
// One thread per pair of fine columns (X, X+1) of one coarse row (iy, iz): it contracts the (one or two) cells' coefficients over xi once,
// then writes the pair in each of the ry rz fine rows the coarse row covers -- every coefficient is loaded once per pair, not once per
// fine row (across XCDs the fine rows of one coarse row do not share an L2).  Consecutive lanes write consecutive 16-byte pairs of a fine
// row (one non-temporal 16-byte store when `vec`: NX even and `out` 16-byte aligned; else one or two 8-byte stores).  The fine cell
// (X, Y, Z) = (ix rx + a, iy ry + b, iz rz + c) lies at (Z NY + Y) NX + X.  Flux: `phi` = one group's coefficients, out = that group's
// field.  POWER: phi = all ng groups (stride nphi); kappa Sigma_f is constant on the cell, so the groups' x contractions are summed with
// ksf[g*N + e] as weights before the y / z means.  Pairs are walked grid-stride with the (coarse row, pair) position advanced
// incrementally (no 64-bit division per pair).
template <int DIM, int M, bool POWER>
__global__ __launch_bounds__(256) void k_project_refined(const double *__restrict__ phi, const double *__restrict__ ksf, double *__restrict__ out,
                                                         int nx, int ny, long N, long nphi, int ng, int rx, int ry, int rz, int NX, int NY,
                                                         int crows, int npairs, int vec, int step_rows, int step_pairs)
{
    constexpr int nq = (DIM >= 2 ? M + 1 : 1) * (DIM == 3 ? M + 1 : 1);
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x;
    int row = (int)(i0 / npairs), pr = (int)(i0 - (long)row * npairs);
    while (row < crows) {
        const int iz = row / ny, iy = row - iz * ny;
        const int X0 = 2 * pr;
        const bool two = X0 + 1 < NX;
        const int ix0 = X0 / rx, ix1 = (X0 + 1) / rx;
        double A0[M + 1], A1[M + 1];
        sub_means<M>(X0 - ix0 * rx, rx, A0);
        sub_means<M>(X0 + 1 - ix1 * rx, rx, A1);
        const long e0 = (long)row * nx + ix0, e1 = (long)row * nx + (two ? ix1 : ix0);
        double s0[nq], s1[nq];
        for (int g = 0; g < (POWER ? ng : 1); ++g) {
            const double *c = phi + (long)g * nphi;
            double t0[nq], t1[nq], u[nq];
            x_contract2<DIM, M>(c, N, e0, A0, A1, t0, t1);
            if (e1 != e0) x_contract2<DIM, M>(c, N, e1, A1, A1, t1, u);
            const double k0 = POWER ? ksf[(long)g * N + e0] : 1.0, k1 = POWER ? ksf[(long)g * N + e1] : 1.0;
#pragma unroll
            for (int q = 0; q < nq; ++q) {
                if (!POWER) { s0[q] = t0[q]; s1[q] = t1[q]; }
                else if (g == 0) { s0[q] = k0 * t0[q]; s1[q] = k1 * t1[q]; }
                else { s0[q] += k0 * t0[q]; s1[q] += k1 * t1[q]; }
            }
        }
        for (int cz = 0; cz < rz; ++cz) {
            double Cz[M + 1];
            sub_means<M>(cz, rz, Cz);
            for (int b = 0; b < ry; ++b) {
                double B[M + 1];
                sub_means<M>(b, ry, B);
                const double v0 = yz_contract<DIM, M>(s0, B, Cz), v1 = yz_contract<DIM, M>(s1, B, Cz);
                const long o = ((long)(iz * rz + cz) * NY + (iy * ry + b)) * NX + X0;
                if (vec) { nf_d2 v = { v0, v1 }; __builtin_nontemporal_store(v, reinterpret_cast<nf_d2 *>(out + o)); }
                else { __builtin_nontemporal_store(v0, out + o); if (two) __builtin_nontemporal_store(v1, out + o + 1); }
            }
        }
        pr += step_pairs; row += step_rows;                       // advance by the grid's stride: step_rows rows + step_pairs pairs
        if (pr >= npairs) { pr -= npairs; ++row; }
    }
}

// ---- zoom: the coarse solution's fission source as the load vector of the refined mesh (nf_zoom_source) -------------------
// Legendre coefficients of a polynomial of degree M on sub-interval s of r equal parts of [-1, 1]: c'_i' = sum_i T[i'][i] c_i, T upper
// triangular, row-major (M+1) x (M+1).  With [al, be] as in sub_means, mu = (al + be) / 2, w = 1 / r:
// T = [[1, mu, (3 mu^2 + w^2 - 1) / 2], [0, w, 3 mu w], [0, 0, w^2]]; row 0 is sub_means itself.  r = 1 gives the identity exactly.
template <int M>
__device__ __forceinline__ void sub_restrict(int s, int r, double *T)
{
    sub_means<M>(s, r, T);
    if (M >= 1) {
        const double w = 1.0 / (double)r, mu = T[1];
        T[(M + 1) + 0] = 0.0; T[(M + 1) + 1] = w;
        if (M >= 2) { T[(M + 1) + 2] = 3.0 * mu * w; T[2 * (M + 1) + 0] = 0.0; T[2 * (M + 1) + 1] = 0.0; T[2 * (M + 1) + 2] = w * w; }
    }
}
// t[p] = sum_g w[g*N + e] c_g[p*N + e] over the ng groups (c = all groups' coefficients, stride nphi): one load per coefficient and weight
template <int NLOC>
__device__ __forceinline__ void zoom_contract(const double *__restrict__ c, const double *__restrict__ w, long N, long nphi, int ng, long e, double *t)
{
#pragma unroll
    for (int p = 0; p < NLOC; ++p) t[p] = 0.0;
    for (int g = 0; g < ng; ++g) {
        const double wg = w[(long)g * N + e];
        const double *cg = c + (long)g * nphi + e;
#pragma unroll
        for (int p = 0; p < NLOC; ++p) t[p] += wg * cg[(long)p * N];
    }
}
// the x restriction in place: t[i' + n1 q] = sum_{i >= i'} T[i'][i] t[i + n1 q] (ascending i' only reads entries not yet overwritten)
template <int DIM, int M>
__device__ __forceinline__ void zoom_restrict_x(double *t, const double *T)
{
    constexpr int n1 = M + 1, nq = (DIM >= 2 ? n1 : 1) * (DIM == 3 ? n1 : 1);
#pragma unroll
    for (int q = 0; q < nq; ++q)
#pragma unroll
        for (int ip = 0; ip <= M; ++ip) {
            double v = T[ip * n1 + ip] * t[ip + n1 * q];
#pragma unroll
            for (int i = ip + 1; i <= M; ++i) v += T[ip * n1 + i] * t[i + n1 * q];
            t[ip + n1 * q] = v;
        }
}
// moment (i', j', k') of the fine cell from the x-restricted values u: sum_{j >= j', k >= k'} Ty[j'][j] Tz[k'][k] u[i' + n1 j + n1^2 k]
template <int DIM, int M>
__device__ __forceinline__ double zoom_restrict_yz(const double *u, const double *Ty, const double *Tz, int ip, int jp, int kp)
{
    constexpr int n1 = M + 1;
    if (DIM == 1) return u[ip];
    double v = 0.0;
#pragma unroll
    for (int k = 0; k <= (DIM == 3 ? M : 0); ++k)
#pragma unroll
        for (int j = 0; j <= M; ++j)
            if (j >= jp && k >= kp) v += (Ty[jp * n1 + j] * (DIM == 3 ? Tz[kp * n1 + k] : 1.0)) * u[ip + n1 * j + n1 * n1 * k];
    return v;
}
// q_g[E, p'] = wout_g(e) inv_k |E| prod_t 1 / (2 i'_t + 1) * (restriction to E of sum_g' win_g'(e) c_g'(e))[p'] for every fine cell E of the
// mesh refined by (rx, ry, rz), every group g and every moment p': the fine mesh's fission-matrix entry nuSigf |E| C-hat_p'p' (k_cell_coef,
// without its 1e-14 drop) times the restricted coefficient, summed over the source groups and scaled by chi_g / k.  Direct: win = nuSigf,
// wout = chi; adjoint: win = chi, wout = nuSigf (both [g*N + e] on the COARSE mesh: a fine cell has its parent's cross sections).
// Shaped like k_project_refined: a thread owns a pair of fine columns (X, X+1) of one coarse row.  It contracts the ng groups' coefficients
// with the in-weights once per coarse cell (one load per coefficient and pair), restricts over xi once, and then, group by group, walks the
// ry rz fine rows applying the y / z restrictions -- the arithmetic of a row is redone per group (at most 9 FMAs per value), the loads are
// not.  Output in the fine handle's device layout q[g*nphiF + p'*NF + E], E = (Z NY + Y) NX + X: one 16-byte store per pair when `vec`
// (NX even: every offset g*nphiF + p'*NF + row*NX + X0 is then even), else 8-byte stores.  Fine indices are 64-bit.
// flags: bit 0 is raised once a non-zero value was written, bit 1 for a non-finite one (read first: after the first waves nobody writes).
// part[block] = the block's share of sum_g sum_E q_g[E, dof 0], the source total of nf_zoom_result (k_zoom_total adds the shares up).
template <int DIM, int M>
__global__ __launch_bounds__(256) void k_zoom_source(const double *__restrict__ phi, const double *__restrict__ win, const double *__restrict__ wout,
                                                     double *__restrict__ q, const double *__restrict__ hx, const double *__restrict__ hy,
                                                     const double *__restrict__ hz, double inv_k, int nx, int ny, long N, long nphi, int ng,
                                                     int rx, int ry, int rz, int NX, int NY, long NF, int crows, int npairs, int vec,
                                                     int step_rows, int step_pairs, int *__restrict__ flags, double *__restrict__ part)
{
    __shared__ double sred[4];
    double tot = 0.0;
    constexpr int n1 = M + 1, nj = DIM >= 2 ? n1 : 1, nk = DIM == 3 ? n1 : 1, nloc = n1 * nj * nk;
    const long nphiF = (long)nloc * NF;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x;
    int row = (int)(i0 / npairs), pr = (int)(i0 - (long)row * npairs);
    int seen = 0;
    while (row < crows) {
        const int iz = row / ny, iy = row - iz * ny;
        const int X0 = 2 * pr;
        const bool two = X0 + 1 < NX;
        const int ix0 = X0 / rx, ix1 = two ? (X0 + 1) / rx : ix0;
        const long e0 = (long)row * nx + ix0, e1 = (long)row * nx + ix1;
        double u0[nloc], u1[nloc], T[n1 * n1];
        zoom_contract<nloc>(phi, win, N, nphi, ng, e0, u0);
        if (e1 != e0) zoom_contract<nloc>(phi, win, N, nphi, ng, e1, u1);
        else {
#pragma unroll
            for (int p = 0; p < nloc; ++p) u1[p] = u0[p];
        }
        sub_restrict<M>(X0 - ix0 * rx, rx, T); zoom_restrict_x<DIM, M>(u0, T);
        sub_restrict<M>((two ? X0 + 1 : X0) - ix1 * rx, rx, T); zoom_restrict_x<DIM, M>(u1, T);
        const double vyz = (DIM >= 2 ? hy[iy] / (double)ry : 1.0) * (DIM == 3 ? hz[iz] / (double)rz : 1.0);   // |E| = |e| / (rx ry rz)
        const double V0 = hx[ix0] / (double)rx * vyz, V1 = hx[ix1] / (double)rx * vyz;
        for (int g = 0; g < ng; ++g) {
            const double s0 = wout[(long)g * N + e0] * inv_k * V0, s1 = wout[(long)g * N + e1] * inv_k * V1;
            double *qg = q + (long)g * nphiF;
            for (int cz = 0; cz < rz; ++cz) {
                double Tz[n1 * n1];
                sub_restrict<M>(cz, rz, Tz);
                for (int b = 0; b < ry; ++b) {
                    double Ty[n1 * n1];
                    sub_restrict<M>(b, ry, Ty);
                    const long o = ((long)(iz * rz + cz) * NY + (iy * ry + b)) * NX + X0;
#pragma unroll
                    for (int kp = 0; kp < nk; ++kp)
#pragma unroll
                        for (int jp = 0; jp < nj; ++jp)
#pragma unroll
                            for (int ip = 0; ip < n1; ++ip) {
                                const int p = ip + n1 * jp + n1 * nj * kp;
                                const double ch = 1.0 / (double)((2 * ip + 1) * (2 * jp + 1) * (2 * kp + 1));   // C-hat_pp detJ' = |E| ch
                                const double v0 = (s0 * ch) * zoom_restrict_yz<DIM, M>(u0, Ty, Tz, ip, jp, kp);
                                const double v1 = (s1 * ch) * zoom_restrict_yz<DIM, M>(u1, Ty, Tz, ip, jp, kp);
                                double *dst = qg + (long)p * NF + o;
                                if (vec) { nf_d2 v = { v0, v1 }; __builtin_nontemporal_store(v, reinterpret_cast<nf_d2 *>(dst)); }
                                else { __builtin_nontemporal_store(v0, dst); if (two) __builtin_nontemporal_store(v1, dst + 1); }
                                if (p == 0) tot += two ? v0 + v1 : v0;
                                if (v0 != 0.0 || (two && v1 != 0.0)) seen |= 1;
                                if (!isfinite(v0) || (two && !isfinite(v1))) seen |= 2;
                            }
                }
            }
        }
        pr += step_pairs; row += step_rows;                       // advance by the grid's stride: step_rows rows + step_pairs pairs
        if (pr >= npairs) { pr -= npairs; ++row; }
    }
    if (seen & ~__hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(flags, seen);
    tot = block_sum(tot, sred);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// one block: *out = the sum of the n block shares k_zoom_source left in part (a fixed order: the total is reproducible)
__global__ __launch_bounds__(256) void k_zoom_total(const double *__restrict__ part, int n, double *__restrict__ out)
{
    __shared__ double sred[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    s = block_sum(s, sred);
    if (threadIdx.x == 0) *out = s;
}

// ---- sensitivity maps: dk/dXS per cell from the direct and the adjoint flux (nf_sensitivity) ------------------------------
// With m[g,g',e] = sum_p phi+_g[e,p] W_p(e) phi_g'[e,p], W_p(e) = |e| / prod_t (2 p_t + 1) (the build's mass weight detJ C-hat_pp of a unit
// cross section), Nrm = phi+^T F phi = sum chi_g nuSigf_g' m[g,g',e] and c = -k^2 / Nrm.  The build's 1e-14 drop thresholds (chi / k, the
// scatter blocks, the RT0 cell_a entries) are ignored: the maps are the derivatives of the operator without them.
// (ix, iy, iz) of cell e by 32-bit division (nf_sensitivity refuses meshes of 2^32 cells or more)
__device__ __forceinline__ void sens_cell(long e, int nx, int ny, int &ix, int &iy, int &iz)
{
    const unsigned u = (unsigned)e, row = u / (unsigned)nx;
    ix = (int)(u - row * (unsigned)nx); iz = (int)(row / (unsigned)ny); iy = (int)(row - (unsigned)iz * (unsigned)ny);
}
template <int DIM>
__device__ __forceinline__ double sens_volume(const double *__restrict__ hx, const double *__restrict__ hy, const double *__restrict__ hz, int ix, int iy, int iz)
{
    return hx[ix] * (DIM >= 2 ? hy[iy] : 1.0) * (DIM == 3 ? hz[iz] : 1.0);
}
// 1 / prod_t (2 p_t + 1) of moment p = i + n1 j + n1^2 k (a constant once the loop over p is unrolled)
template <int DIM, int M>
__device__ __forceinline__ double sens_ch(int p)
{
    constexpr int n1 = M + 1;
    const int i = p % n1, j = DIM >= 2 ? (p / n1) % n1 : 0, k = DIM == 3 ? p / (n1 * n1) : 0;
    return 1.0 / (double)((2 * i + 1) * (2 * j + 1) * (2 * k + 1));
}
// Nrm factorises: sum_{e,p} W_p (sum_g chi_g phi+_g)[e,p] (sum_g' nuSigf_g' phi_g')[e,p].  part[block] = the block's share; k_sens_scalars
// adds the shares in a fixed order (the two-stage pattern of every reduction here: the total is reproducible)
template <int DIM, int M>
__global__ __launch_bounds__(256) void k_sens_norm(const double *__restrict__ phi, const double *__restrict__ adj, const double *__restrict__ chi,
                                                   const double *__restrict__ nsf, const double *__restrict__ hx, const double *__restrict__ hy,
                                                   const double *__restrict__ hz, int nx, int ny, long N, long nphi, int ng, double *__restrict__ part)
{
    __shared__ double sred[4];
    constexpr int n1 = M + 1, nloc = n1 * (DIM >= 2 ? n1 : 1) * (DIM == 3 ? n1 : 1);
    double tot = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        int ix, iy, iz; sens_cell(e, nx, ny, ix, iy, iz);
        const double vol = sens_volume<DIM>(hx, hy, hz, ix, iy, iz);
        double s1[nloc], s2[nloc];
#pragma unroll
        for (int p = 0; p < nloc; ++p) { s1[p] = 0.0; s2[p] = 0.0; }
        for (int g = 0; g < ng; ++g) {
            const double cg = chi[(long)g * N + e], fg = nsf[(long)g * N + e];
            const double *a = adj + (long)g * nphi + e, *f = phi + (long)g * nphi + e;
#pragma unroll
            for (int p = 0; p < nloc; ++p) { s1[p] += cg * a[(long)p * N]; s2[p] += fg * f[(long)p * N]; }
        }
        double v = 0.0;
#pragma unroll
        for (int p = 0; p < nloc; ++p) v += (vol * sens_ch<DIM, M>(p)) * (s1[p] * s2[p]);
        tot += v;
    }
    tot = block_sum(tot, sred);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// one block: sc[0] = Nrm (the n shares added in a fixed order), sc[1] = c = -k^2 / Nrm, sc[2] = -c / k; they stay on the device for the
// map kernels (the host reads sc[0] for the result struct and the error check only)
__global__ __launch_bounds__(256) void k_sens_scalars(const double *__restrict__ part, int n, double keff, double *__restrict__ sc)
{
    __shared__ double sred[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    s = block_sum(s, sred);
    if (threadIdx.x == 0) { const double c = -(keff * keff) / s; sc[0] = s; sc[1] = c; sc[2] = -c / keff; }
}
// One thread per cell, one streaming pass: dSigR[g,e] = c m[g,g,e], dSigS[(g*ng+g')*N+e] = -c m[g,g',e] (0 for g' = g: the solver never
// reads the diagonal), dNSF[g',e] = -(c/k) sum_p W_p phi_g'[p] s1[p], dChi[g,e] = -(c/k) sum_p W_p phi+_g[p] s2[p] with the factorised sums
// s1 = sum_g chi_g phi+_g, s2 = sum_g' nuSigf_g' phi_g' (formed once per cell: the ng^2 products only where dSigS asks for them).  Fields in
// the device SoA layout [g*nphi + p*N + e]: consecutive lanes read and write consecutive doubles in every stream.  Every output is written
// once, already scaled by the device-resident c, with non-temporal stores; a NULL output is skipped (the others are computed by the same
// instructions: they come out bit-identical).  ng is a run-time loop: a group's coefficients are read again (from L2) when dSigS pairs it
// with another group.
template <int DIM, int M>
__global__ __launch_bounds__(256) void k_sens_mass(const double *__restrict__ phi, const double *__restrict__ adj, const double *__restrict__ chi,
                                                   const double *__restrict__ nsf, const double *__restrict__ hx, const double *__restrict__ hy,
                                                   const double *__restrict__ hz, int nx, int ny, long N, long nphi, int ng,
                                                   const double *__restrict__ sc, double *__restrict__ dSigR, double *__restrict__ dNSF,
                                                   double *__restrict__ dChi, double *__restrict__ dSigS)
{
    constexpr int n1 = M + 1, nloc = n1 * (DIM >= 2 ? n1 : 1) * (DIM == 3 ? n1 : 1);
    const double c = sc[1], ck = sc[2];
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        int ix, iy, iz; sens_cell(e, nx, ny, ix, iy, iz);
        const double vol = sens_volume<DIM>(hx, hy, hz, ix, iy, iz);
        double s1[nloc], s2[nloc];
#pragma unroll
        for (int p = 0; p < nloc; ++p) { s1[p] = 0.0; s2[p] = 0.0; }
        if (dNSF || dChi)
            for (int g = 0; g < ng; ++g) {
                const double cg = chi[(long)g * N + e], fg = nsf[(long)g * N + e];
                const double *a = adj + (long)g * nphi + e, *f = phi + (long)g * nphi + e;
#pragma unroll
                for (int p = 0; p < nloc; ++p) { s1[p] += cg * a[(long)p * N]; s2[p] += fg * f[(long)p * N]; }
            }
        for (int g = 0; g < ng; ++g) {
            const double *a = adj + (long)g * nphi + e, *f = phi + (long)g * nphi + e;
            double wa[nloc];                                      // W_p phi+_g[p], kept for the pairs of dSigS
            double mgg = 0.0, vn = 0.0, vc = 0.0;
#pragma unroll
            for (int p = 0; p < nloc; ++p) {
                const double w = vol * sens_ch<DIM, M>(p), fp = f[(long)p * N];
                wa[p] = w * a[(long)p * N];
                mgg += wa[p] * fp; vn += (w * fp) * s1[p]; vc += wa[p] * s2[p];
            }
            if (dSigR) __builtin_nontemporal_store(c * mgg, dSigR + (long)g * N + e);
            if (dNSF) __builtin_nontemporal_store(ck * vn, dNSF + (long)g * N + e);
            if (dChi) __builtin_nontemporal_store(ck * vc, dChi + (long)g * N + e);
            if (dSigS)
                for (int gp = 0; gp < ng; ++gp) {
                    double v = 0.0;
                    if (gp != g) {
                        const double *fo = phi + (long)gp * nphi + e;
#pragma unroll
                        for (int p = 0; p < nloc; ++p) v += wa[p] * fo[(long)p * N];
                        v = -c * v;
                    }
                    __builtin_nontemporal_store(v, dSigS + ((long)g * ng + gp) * N + e);
                }
        }
    }
}
// One thread per cell and one group per launch: dD[e] = c (a / D(e)^2 - 2 b) from the two currents j = A^-1 B^T phi_g and j+ = A^-1 B^T phi+_g
// in the reference DOF order (k_flux_to_J; its sign cancels in every product).  Per direction d the 2 nf + ni local current DOFs decouple
// into one chain of 2 + K unknowns (lower face, upper face, K bubbles) per transverse mode a, coupled by T_a times the 1-D matrix of
// {(1-s)/2, (1+s)/2, (1-s^2) P_l(s)} (src/FEM.cpp:891-924, exact under the reference's quadrature):
//   a = sum_d factor_d(e) sum_a T_a j+_a^T A1 j_a,   A1 = [[2/3, 1/3, 2/3, -2/15], [1/3, 2/3, 2/3, 2/15], [2/3, 2/3, 16/15, 0], [-2/15, 2/15, 0, 16/105]]
//   b = sum over the Dirichlet boundary faces f of e and their modes of I_f(a) j+_{f,a} j_{f,a},  I_f(a) = T_a dirichlet_term / (2 D)
// Face DOF (face, a) at face*nfa + a in the direction's face block (offsets foff), bubble (l, a) of cell e at e*ni + l + K a in its bubble
// block; the faces of consecutive cells of a row are consecutive in x and a row apart in y / z: all three directions are read coalesced
// across ix (with stride nfa doubles).  dD is written once, non-temporally.
struct SensJ { long foff[3]; long boff[3]; };
template <int DIM, int K>
__global__ __launch_bounds__(256) void k_sens_current(Geom G, SensJ O, const double *__restrict__ j, const double *__restrict__ ja,
                                                      const double *__restrict__ D, const double *__restrict__ sc, long N, double *__restrict__ dD)
{
    constexpr int nfa = (DIM >= 2 ? K + 1 : 1) * (DIM == 3 ? K + 1 : 1), ni = K * nfa;
    constexpr int UNR = nfa <= 3 ? nfa : 1;                       // 3D, K >= 1: the 4 / 9 modes one after the other (unrolled they hold 196 / 490 registers)
    const double c = sc[1];
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        int ix, iy, iz; sens_cell(e, G.nx, G.ny, ix, iy, iz);
        double av = 0.0, bv = 0.0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            const long flo = cmfd_face(G, d, ix, iy, iz);
            const long fhi = flo + (d == 0 ? 1L : d == 1 ? (long)G.nx : (long)G.nx * G.ny);
            const int ci = d == 0 ? ix : d == 1 ? iy : iz, n = d == 0 ? G.nx : d == 1 ? G.ny : G.nz;
            const bool dlo = ci == 0 && G.dir_lo[d], dhi = ci == n - 1 && G.dir_hi[d];
            const double area = d == 0 ? G.hy[iy] * G.hz[iz] : d == 1 ? G.hx[ix] * G.hz[iz] : G.hx[ix] * G.hy[iy];
            const double I = DIM == 1 ? 1.0 : DIM == 2 ? 2.0 / area : 4.0 / area;
            double q = 0.0, bq = 0.0;
#pragma unroll UNR
            for (int a = 0; a < nfa; ++a) {
                const double Ta = DIM == 1 ? 1.0 : DIM == 2 ? 2.0 / (2 * a + 1) : (2.0 / (2 * (a % (K + 1)) + 1)) * (2.0 / (2 * (a / (K + 1)) + 1));
                const double uL = j[O.foff[d] + flo * nfa + a], uR = j[O.foff[d] + fhi * nfa + a];
                const double vL = ja[O.foff[d] + flo * nfa + a], vR = ja[O.foff[d] + fhi * nfa + a];
                double t = vL * (2.0 / 3.0 * uL + 1.0 / 3.0 * uR) + vR * (1.0 / 3.0 * uL + 2.0 / 3.0 * uR);
                if (K >= 1) {
                    const long bo = O.boff[d] + e * ni + K * a;
                    const double u0 = j[bo], v0 = ja[bo];
                    t += 2.0 / 3.0 * ((vL + vR) * u0 + v0 * (uL + uR)) + 16.0 / 15.0 * (v0 * u0);
                    if (K >= 2) {
                        const double u1 = j[bo + 1], v1 = ja[bo + 1];
                        t += 2.0 / 15.0 * ((vR - vL) * u1 + v1 * (uR - uL)) + 16.0 / 105.0 * (v1 * u1);
                    }
                }
                q += Ta * t;
                bq += Ta * ((dlo ? vL * uL : 0.0) + (dhi ? vR * uR : 0.0));
            }
            av += geom_factor(G, d, ix, iy, iz) * q;
            bv += I * bq;
        }
        const double De = D[e];
        __builtin_nontemporal_store(c * (av / (De * De) - 2.0 * bv), dD + e);
    }
}

// ---------------------------------------------------------------------------------------------
// Block outer iteration (nf_solve_modes): Gram and rotate passes over two blocks of b <= NF_BLOCK_MAX long vectors
// (column-major, leading dimension n).  Both are streaming kernels: every element of every column is read once per tile that needs it.
// Block partials go to rows of `stride` doubles, one entry per block of gridDim.x -- the team partials layout; k_block_finalize sums
// any number of rows in k_finalize's order (k_finalize itself takes four per launch).
static const int NF_BLOCK_MAX = 8, NF_BLOCK_TILE = 4;
// rows of the Gram partials: (Q^T Z)(i, j) at i * b + j, the upper triangle of Z^T Z, i <= j, behind them at b * b + j (j + 1) / 2 + i
__host__ __device__ __forceinline__ int gram_row_qz(int b, int i, int j) { return i * b + j; }
__host__ __device__ __forceinline__ int gram_row_zz(int b, int i, int j) { return b * b + j * (j + 1) / 2 + i; }
// Tile (ti, tj) = blockIdx.y of 4 x 4 entries: columns 4 ti.. of Q (and of Z) against columns 4 tj.. of Z.  The tile forms its part of
// Q^T Z and, for ti <= tj, of Z^T Z from the same loads: 32 accumulators, 8 (diagonal tile) or 12 loads per element.  Full 8 x 8 in one
// thread would need 100 accumulators.  Columns beyond b are clamped to b - 1 (their sums are not stored).
__global__ __launch_bounds__(256) void k_block_gram(const double *__restrict__ Q, const double *__restrict__ Z, int b, long n,
                                                    double *__restrict__ partials, long stride)
{
    constexpr int TW = NF_BLOCK_TILE;
    __shared__ double sred[4];
    const int nt = (b + TW - 1) / TW, ti = blockIdx.y / nt, tj = blockIdx.y % nt;
    const bool zz = ti <= tj, diag = ti == tj;
    const double *qi[TW], *zi[TW], *zj[TW];
#pragma unroll
    for (int a = 0; a < TW; ++a) {
        const int ci = min(ti * TW + a, b - 1), cj = min(tj * TW + a, b - 1);
        qi[a] = Q + (long)ci * n; zi[a] = Z + (long)ci * n; zj[a] = Z + (long)cj * n;
    }
    double h[TW][TW], g[TW][TW];
#pragma unroll
    for (int a = 0; a < TW; ++a)
#pragma unroll
        for (int c = 0; c < TW; ++c) { h[a][c] = 0.0; g[a][c] = 0.0; }
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += gridDim.x * 256L) {
        double q[TW], zc[TW], zr[TW];
#pragma unroll
        for (int a = 0; a < TW; ++a) { q[a] = qi[a][e]; zc[a] = zj[a][e]; }
        if (zz && !diag) {
#pragma unroll
            for (int a = 0; a < TW; ++a) zr[a] = zi[a][e];
        } else {
#pragma unroll
            for (int a = 0; a < TW; ++a) zr[a] = zc[a];
        }
#pragma unroll
        for (int a = 0; a < TW; ++a)
#pragma unroll
            for (int c = 0; c < TW; ++c) { h[a][c] = fma(q[a], zc[c], h[a][c]); g[a][c] = fma(zr[a], zc[c], g[a][c]); }
    }
#pragma unroll
    for (int a = 0; a < TW; ++a)
#pragma unroll
        for (int c = 0; c < TW; ++c) {
            const int i = ti * TW + a, j = tj * TW + c;
            const double hs = block_sum(h[a][c], sred), gs = block_sum(g[a][c], sred);
            if (threadIdx.x == 0 && i < b && j < b) {
                partials[gram_row_qz(b, i, j) * stride + blockIdx.x] = hs;
                if (zz && i <= j) partials[gram_row_zz(b, i, j) * stride + blockIdx.x] = gs;
            }
        }
}
// out[row] = sum of the row's `cnt` block partials, in k_finalize's order (strided_sum256 + block_sum); one block per row
__global__ __launch_bounds__(256) void k_block_finalize(const double *__restrict__ partials, long stride, int cnt, double *__restrict__ out)
{
    __shared__ double sred[4];
    double s = strided_sum256(partials + blockIdx.x * stride, cnt);
    s = block_sum(s, sred);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}
// Q <- Z C in place of Q (every output element depends on the same element of the inputs only) and, from the OLD Q of the same loads,
// block partials of the squared column norms of R = Z_m - Q_m H_mm, the invariant-subspace residual of the leading m columns (row j of
// the partials = column j).  C and H: B x B, column-major, H zero outside its leading m x m part -- both in the kernel arguments.
struct BlockCoef { double C[NF_BLOCK_MAX * NF_BLOCK_MAX], H[NF_BLOCK_MAX * NF_BLOCK_MAX]; };
template <int B>
__global__ __launch_bounds__(256) void k_block_rotate(double *Q, const double *__restrict__ Z, int m, long n, BlockCoef cf,
                                                      double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    double r2[B];
#pragma unroll
    for (int j = 0; j < B; ++j) r2[j] = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += gridDim.x * 256L) {
        double q[B], z[B];
#pragma unroll
        for (int l = 0; l < B; ++l) { q[l] = Q[(long)l * n + e]; z[l] = Z[(long)l * n + e]; }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            double v = 0.0, r = z[j];
#pragma unroll
            for (int l = 0; l < B; ++l) { v = fma(z[l], cf.C[l + j * B], v); r = fma(-q[l], cf.H[l + j * B], r); }
            Q[(long)j * n + e] = v;
            r2[j] = fma(r, r, r2[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
        const double s = block_sum(r2[j], sred);
        if (threadIdx.x == 0 && j < m) partials[j * stride + blockIdx.x] = s;
    }
}
// start block of the block iteration: column c = the cosine harmonic (hi, hj, hk)[c] of the cell index,
// cos(pi hi (x + 1/2) / nx) cos(pi hj (y + 1/2) / ny) cos(pi hk (z + 1/2) / nz), the same in every group, zero in the higher moments
// (device DOF order [p][e]: the cell means are the first N entries of a group)
struct StartArgs { int hi[NF_BLOCK_MAX], hj[NF_BLOCK_MAX], hk[NF_BLOCK_MAX]; };
__global__ __launch_bounds__(256) void k_modes_start(double *__restrict__ Z, int b, int ng, long nphi, long N, int nx, int ny, int nz, StartArgs sa)
{
    const long nt = (long)ng * nphi, total = nt * b;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i / nt);
        const long d = (i - c * nt) % nphi;
        double v = 0.0;
        if (d < N) {
            const int ix = (int)(d % nx); const long r = d / nx; const int iy = (int)(r % ny), iz = (int)(r / ny);
            v = cospi(sa.hi[c] * (ix + 0.5) / nx) * cospi(sa.hj[c] * (iy + 0.5) / ny) * cospi(sa.hk[c] * (iz + 0.5) / nz);
        }
        Z[i] = v;
    }
}
// the returned vectors of nf_solve_modes from the last application of A: x_i = sum_l q_l Wz[l, i] (written to X), its residual
// r_i = sum_l z_l Wz[l, i] - sum_l q_l Wq[l, i] (Wq = Wz Theta, Theta the real block form of the eigenvalues), and block partials of
// |x_i|^2 (rows 0..7), |r_i|^2 (8..15), sum w x_i (16..23) and sum |w x_i| (24..31) with w the fission (adjoint: chi-weighted mass)
// diagonal over all groups.  Coefficients 8 x 8 column-major, zero beyond m; columns beyond m are clamped (their sums are ignored).
struct ExtractCoef { double Wz[NF_BLOCK_MAX * NF_BLOCK_MAX], Wq[NF_BLOCK_MAX * NF_BLOCK_MAX]; };
__global__ __launch_bounds__(256) void k_modes_extract(const double *__restrict__ Q, const double *__restrict__ Z, int m, long n,
                                                       const double *__restrict__ w, ExtractCoef cf, double *__restrict__ X,
                                                       double *__restrict__ partials, long stride)
{
    constexpr int B = NF_BLOCK_MAX;
    __shared__ double sred[4];
    double acc[4][B];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < B; ++j) acc[t][j] = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += gridDim.x * 256L) {
        double q[B], z[B];
        const double we = w[e];
#pragma unroll
        for (int l = 0; l < B; ++l) { const long c = min(l, m - 1); q[l] = Q[c * n + e]; z[l] = Z[c * n + e]; }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            double x = 0.0, r = 0.0;
#pragma unroll
            for (int l = 0; l < B; ++l) { x = fma(q[l], cf.Wz[l + j * B], x); r = fma(z[l], cf.Wz[l + j * B], r); r = fma(-q[l], cf.Wq[l + j * B], r); }
            if (j < m) X[(long)j * n + e] = x;
            acc[0][j] = fma(x, x, acc[0][j]); acc[1][j] = fma(r, r, acc[1][j]); acc[2][j] = fma(we, x, acc[2][j]); acc[3][j] += fabs(we * x);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const double s = block_sum(acc[t][j], sred);
            if (threadIdx.x == 0) partials[(t * B + j) * stride + blockIdx.x] = s;
        }
}

// ---- generalized adjoint and response-ratio maps (nf_solve_gpt / nf_gpt_sensitivity) ------------------------------------
// Streaming grid-stride kernels over the device SoA layout [g*n + p*N + e] (n = DOFs per group): blockIdx.y is the group, blockIdx.x walks
// the group's n DOFs (no division by n per element), block (x, y) writes its partial at y * gridDim.x + x of a row of `stride` doubles;
// k_block_finalize adds a row's gridDim.x * gridDim.y partials in a fixed order and the totals stay on the device in the slots below.
enum { GPT_WA = 0, GPT_WB = 1, GPT_DEN = 2, GPT_FF = 3, GPT_NUM = 4, GPT_NN = 5, GPT_DD = 6, GPT_SLOTS = 8 };
// <w_a, phi> (row 0) and <w_b, phi> (row 1), <w, phi> = sum_g sum_e w[g,e] |e| phibar_g(e): one pass over the DOF-0 rows of all groups
__global__ __launch_bounds__(256) void k_gpt_response(const double *__restrict__ phi, const double *__restrict__ wa, const double *__restrict__ wb,
                                                      const double *__restrict__ hx, const double *__restrict__ hy, const double *__restrict__ hz,
                                                      int nx, int ny, long N, long n, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    const long g = blockIdx.y;
    double sa = 0.0, sb = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < N; e += gridDim.x * 256L) {
        const double v = cell_measure(hx, hy, hz, nx, ny, e) * phi[g * n + e];
        sa = fma(wa[g * N + e], v, sa); sb = fma(wb[g * N + e], v, sb);
    }
    sa = block_sum(sa, sred); sb = block_sum(sb, sred);
    if (threadIdx.x == 0) { const long b = (long)blockIdx.y * gridDim.x + blockIdx.x; partials[b] = sa; partials[stride + b] = sb; }
}
// S+ = w_a |e| / <w_a, phi> - w_b |e| / <w_b, phi> on the DOF-0 rows, 0 on the higher moments (src; may be NULL), from the device-resident
// sums sc[GPT_WA], sc[GPT_WB]; with dWa / dWb (may be NULL) the direct maps (1/R) dR/dw_a = |e| phibar / <w_a, phi> and
// (1/R) dR/dw_b = -|e| phibar / <w_b, phi>, [g*N + e]
__global__ __launch_bounds__(256) void k_gpt_source(const double *__restrict__ phi, const double *__restrict__ wa, const double *__restrict__ wb,
                                                    const double *__restrict__ sc, const double *__restrict__ hx, const double *__restrict__ hy,
                                                    const double *__restrict__ hz, int nx, int ny, long N, long n, double *__restrict__ src,
                                                    double *__restrict__ dWa, double *__restrict__ dWb)
{
    const long g = blockIdx.y;
    const double A = sc[GPT_WA], B = sc[GPT_WB];
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n; j += gridDim.x * 256L) {
        if (j >= N) { if (src) src[g * n + j] = 0.0; continue; }
        const double vol = cell_measure(hx, hy, hz, nx, ny, j);
        if (src) src[g * n + j] = wa[g * N + j] * vol / A - wb[g * N + j] * vol / B;
        if (dWa || dWb) {
            const double v = vol * phi[g * n + j];
            if (dWa) __builtin_nontemporal_store(v / A, dWa + g * N + j);
            if (dWb) __builtin_nontemporal_store(-(v / B), dWb + g * N + j);
        }
    }
}
// <x, F phi> (row 0) and ||F phi||^2 (row 1) in one pass over x: (F phi)_g[p, e] = chi_g(e) tf[p, e] with tf = sum_g' Mf_g' phi_g' (k_fission),
// formed on the fly -- F phi is never stored.  x = Gamma: the numerator of the deflation; x = phi+: its denominator, once per call.
__global__ __launch_bounds__(256) void k_gpt_defl_dot(const double *__restrict__ x, const double *__restrict__ chi, const double *__restrict__ tf,
                                                      long N, long n, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    const long g = blockIdx.y;
    double s = 0.0, ff = 0.0;
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n; j += gridDim.x * 256L) {
        const long e = n == N ? j : j % N;
        const double f = chi[g * N + e] * tf[j];
        s = fma(x[g * n + j], f, s); ff = fma(f, f, ff);
    }
    s = block_sum(s, sred); ff = block_sum(ff, sred);
    if (threadIdx.x == 0) { const long b = (long)blockIdx.y * gridDim.x + blockIdx.x; partials[b] = s; partials[stride + b] = ff; }
}
// Gamma -= beta phi+ with beta = sc[GPT_NUM] / sc[GPT_DEN] read from the device (no host round trip), the block partials of ||Gamma||^2
// (row 0) and ||Gamma - old||^2 (row 1) of the deflated iterate, and old <- Gamma, all in one sweep (the shape of k_subcrit_reduce):
// three loads and two stores per DOF
__global__ __launch_bounds__(256) void k_gpt_defl_update(double *__restrict__ gamma, const double *__restrict__ adj, double *__restrict__ old,
                                                         const double *__restrict__ sc, long n, double *__restrict__ partials, long stride)
{
    __shared__ double sred[4];
    const long g = blockIdx.y;
    const double beta = sc[GPT_NUM] / sc[GPT_DEN];
    double sn = 0.0, sd = 0.0;
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n; j += gridDim.x * 256L) {
        const long i = g * n + j;
        const double v = fma(-beta, adj[i], gamma[i]), d = v - old[i];
        gamma[i] = v; old[i] = v;
        sn = fma(v, v, sn); sd = fma(d, d, sd);
    }
    sn = block_sum(sn, sred); sd = block_sum(sd, sred);
    if (threadIdx.x == 0) { const long b = (long)blockIdx.y * gridDim.x + blockIdx.x; partials[b] = sn; partials[stride + b] = sd; }
}
// one block, the counterpart of k_sens_scalars for the response ratio: sc[0] = <Gamma+, F phi> as measured (the n partials of a
// k_gpt_defl_dot row added in k_block_finalize's order; it is reported, the maps do not divide by it), sc[1] = c = -1, sc[2] = -c / k = 1 / k.
// k_sens_mass and k_sens_current then run unchanged on (phi, Gamma+).
__global__ __launch_bounds__(256) void k_gpt_scalars(const double *__restrict__ part, int n, double keff, double *__restrict__ sc)
{
    __shared__ double sred[4];
    double s = strided_sum256(part, n);
    s = block_sum(s, sred);
    if (threadIdx.x == 0) { sc[0] = s; sc[1] = -1.0; sc[2] = 1.0 / keff; }
}

// fill with a deterministic pseudo-random pattern (profiling helper)
__global__ void k_fill_pattern(double *__restrict__ v, long n)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        unsigned long long s = (unsigned long long)i * 6364136223846793005ULL + 1442695040888963407ULL;
        s ^= s >> 29;
        v[i] = (double)(s & 0xFFFFFF) / 16777216.0 - 0.5;
    }
}

}  // namespace nf
