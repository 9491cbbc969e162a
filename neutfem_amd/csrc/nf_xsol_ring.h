// Ring of CG directions behind the batched x_sol update of the fused form (CgFuse in nf_kernels.h).  x_sol is the one vector a CG iteration
// never reads back, so the x pass need not touch it every time: the direction p_k of iteration k goes into slot k % M of a ring of M buffers,
// and only the x pass of every M-th iteration applies x_sol = fma(alpha_j, p_j, x_sol) for the M directions since the last time, oldest
// first -- the same chain of fma per cell, the same bits.  What is still pending when the solve ends, k_cg_flush applies.
// Everything here is a pure function of the iteration index k (cg_step's `index`) and M.  Plain C++: no device code, so that it can be
// built and run on its own (tests/host/xsol_ring_main.cpp).
#pragma once

constexpr int NF_XSOL_RING_MAX = 8;                               // largest M = entries of the alpha history (cg_logic)

struct NfRingUpdate { int slot, alpha; };                         // x_sol = fma(ah[alpha], ring[slot], x_sol)
struct NfRingBatch { int n = 0; NfRingUpdate u[NF_XSOL_RING_MAX] = {}; };   // in the order they are applied

// FIN_PAP of iteration j stores alpha_j here (cg->its == j at that point)
inline int nf_ring_alpha(long j) { return (int)(j % NF_XSOL_RING_MAX); }
// The x pass of iteration k reads p_{k-1} (k = 0: p_0 as the start of the solve left it, in slot 0, and writes nothing) ...
inline int nf_ring_read(long k, int M) { return k > 0 ? (int)((k - 1) % M) : 0; }
// ... and writes p_k = r + beta p_{k-1}; the y / z passes of the iteration read it from there.  In a pass that applies a batch this is the
// slot of the batch's oldest direction: a cell is read and written by the same lane, as in the in-place update of M = 1.
inline int nf_ring_write(long k, int M) { return (int)(k % M); }
// the updates alpha_j p_j, lo <= j < hi (at most M of them)
inline NfRingBatch nf_ring_range(long lo, long hi, int M)
{
    NfRingBatch B;
    for (long j = lo; j < hi && B.n < NF_XSOL_RING_MAX; ++j) B.u[B.n++] = { (int)(j % M), nf_ring_alpha(j) };
    return B;
}
// What the x pass of iteration k applies: nothing (n = 0: it neither loads nor stores x_sol), or the M updates k-M .. k-1.  The last of them
// is the direction the pass reads anyway.
inline NfRingBatch nf_ring_apply(long k, int M) { return k >= 1 && k % M == 0 ? nf_ring_range(k - M, k, M) : NfRingBatch(); }
// What a solve that ended with CgScalars::its = n leaves for k_cg_flush.  The solution needs alpha_j p_j for every j < n.  The x passes
// 0 .. n-1 ran; pend = 0 (CgScalars::pend: p.q broke down in iteration n) says that the x pass of iteration n ran as well.  The updates below
// the last multiple of M among them are in x_sol, the rest -- up to M -- still sit in their slots.
inline NfRingBatch nf_ring_pending(long n, int pend, int M)
{
    if (n <= 0) return NfRingBatch();
    const long lastx = pend ? n - 1 : n;
    return nf_ring_range(lastx / M * M, n, M);
}
