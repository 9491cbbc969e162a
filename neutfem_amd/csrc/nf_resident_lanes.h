// The plan of the line-per-lane variants of the resident solve (k_resident_keff<.., NB, PITCH != 0>): which mesh they take, which lane
// slots their directions get and how much LDS they need.  RT0-P0 is the case of one transverse mode.  The mesh is padded to rows of the
// odd length nx | 1.  Plain C++ over plain integers: no HIP headers, no solver structs, so that it can be built and run on its own
// (tests/host/resident_lanes_main.cpp).
#pragma once

// tw[d]: two lanes per line in direction d, meeting in the middle (lines of >= 4 cells); slot0[d]: first lane slot of direction d, each
// direction on a wavefront boundary, slot0[3] = number of slots.  RT0-P0 (nb = 0): pitch of a direction's block, a multiple of 512
// (cells per thread) and of 64 (ds_read2st64).  Bubble moments (nb > 0): PC = cell pitch of a moment, NPp = padded DOFs.  need: LDS in
// doubles -- 64 + 16 in front, the small tables of the bubble variant (176), p, per direction the contribution and {L, 1/d}, three
// per-line values; cap: what a workgroup may have.
struct LanePlan { int tw[3], slot0[4], pitch; long PC, NPp, need; bool fits; };
inline LanePlan lane_plan(int dim, int nx, int ny, int nz, const long nlines[3], int nb, int nloc, int nmodes, bool two_sided, long cap)
{
    LanePlan P = {};
    const long Np = (long)(nx | 1) * ny * nz;                    // rows padded to an odd length (bank-conflict-free x lines)
    const int nm = nb == 0 ? 1 : nmodes;
    long lines = 0; int slot = 0;
    for (int d = 0; d < dim; ++d) {
        const int nd = d == 0 ? nx : d == 1 ? ny : nz;
        P.tw[d] = (nd >= 4 && two_sided) ? 1 : 0;
        lines += (nlines[d] + 1) & ~1L;
        P.slot0[d] = slot; slot += (int)((nlines[d] * nm * (P.tw[d] ? 2 : 1) + 63) / 64) * 64;
    }
    for (int d = dim; d < 4; ++d) P.slot0[d] = slot;
    if (nb == 0) {
        P.pitch = Np <= 1536 ? 1536 : 2560;
        P.need = 64 + 16 + (1 + 3L * dim) * P.pitch + 3 * lines;
        P.fits = Np <= P.pitch && P.need <= cap;
    } else {
        P.PC = (Np + 63) & ~63L; P.NPp = P.PC * nloc;
        P.need = 64 + 16 + 176 + (1 + dim) * P.NPp + 2L * dim * P.PC + 3 * lines;
        P.fits = P.NPp <= 5120 && nmodes <= 9 && nloc <= 27 && P.need <= cap;
    }
    return P;
}
