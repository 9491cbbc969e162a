// Stand-alone check of the plan of the resident solve's line-per-lane variants (neutfem_amd/csrc/nf_resident_lanes.h): the lane slots of a
// set of meshes and the plan's edges, no device.  Meant to be built with -fsanitize=address,undefined as well as plainly; exits non-zero
// on a mismatch.
#include "../../neutfem_amd/csrc/nf_resident_lanes.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; fprintf(stderr, "FAIL %dx%dx%d modes %d two_sided %d: ", nx, ny, nz, nm, (int)two); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return; } } while (0)

static const long BIG = 1L << 40;                                // an LDS that takes everything

// the slots of every direction: on a wavefront boundary, enough for every (mode, line) -- twice that where two lanes share a line --
// and less than a wavefront more; two-sided only from 4 cells on; nothing for the directions the mesh does not have
static void slots(int nx, int ny, int nz, int nm, bool two)
{
    const int dim = nz > 1 ? 3 : ny > 1 ? 2 : 1;
    const long nlines[3] = { (long)ny * nz, (long)nx * nz, (long)nx * ny };
    const int nd[3] = { nx, ny, nz };
    const int nb = nm > 1 ? 1 : 0;                               // RT0-P0 is the case of one mode
    const LanePlan P = lane_plan(dim, nx, ny, nz, nlines, nb, 2 * nm, nm, two, BIG);
    CHECK(P.slot0[0] == 0, "slot0[0] = %d", P.slot0[0]);
    for (int d = 0; d < dim; ++d) {
        CHECK(P.tw[d] == ((two && nd[d] >= 4) ? 1 : 0), "direction %d of %d cells: two-sided %d", d, nd[d], P.tw[d]);
        const long want = nlines[d] * nm * (P.tw[d] ? 2 : 1), have = P.slot0[d + 1] - P.slot0[d];
        CHECK(P.slot0[d] % 64 == 0 && have % 64 == 0 && have >= want && have < want + 64, "direction %d: %ld slots from %d for %ld lanes", d, have, P.slot0[d], want);
    }
    for (int d = dim; d < 3; ++d) CHECK(P.slot0[d + 1] == P.slot0[d] && !P.tw[d], "direction %d beyond the mesh has slots", d);
    // a one-mode bubble mesh gets the slots of the RT0-P0 mesh
    if (nm == 1) {
        const LanePlan Q = lane_plan(dim, nx, ny, nz, nlines, 1, 2, 1, two, BIG);
        for (int d = 0; d < 4; ++d) CHECK(Q.slot0[d] == P.slot0[d] && (d == 3 || Q.tw[d] == P.tw[d]), "bubble plan, direction %d", d);
    }
}

static void plan_edges()
{
    const int nm = 1; const bool two = true;                     // for CHECK's message
    int nx = 0, ny = 0, nz = 1;
    auto rt0 = [&](int x, int y, long cap) { nx = x; ny = y; const long nl[3] = { y, x, 0 }; return lane_plan(2, x, y, 1, nl, 0, 1, 1, true, cap); };
    auto hi = [&](int x, int y, int nloc, int modes, long cap) { nx = x; ny = y; const long nl[3] = { y, x, 0 }; return lane_plan(2, x, y, 1, nl, 1, nloc, modes, true, cap); };
    LanePlan P = rt0(3, 512, BIG);                               // Np = 1536
    CHECK(P.pitch == 1536 && P.fits, "Np = 1536: pitch %d fits %d", P.pitch, (int)P.fits);
    CHECK(P.need == 64 + 16 + 7L * 1536 + 3 * (512 + 4), "Np = 1536: need %ld", P.need);
    P = rt0(29, 53, BIG);                                        // Np = 1537
    CHECK(P.pitch == 2560 && P.fits, "Np = 1537: pitch %d fits %d", P.pitch, (int)P.fits);
    P = rt0(5, 512, BIG);                                        // Np = 2560
    CHECK(P.pitch == 2560 && P.fits, "Np = 2560: pitch %d fits %d", P.pitch, (int)P.fits);
    P = rt0(13, 197, BIG);                                       // Np = 2561
    CHECK(!P.fits, "Np = 2561 fits");
    P = rt0(37, 38, BIG);
    CHECK(rt0(37, 38, P.need).fits && !rt0(37, 38, P.need - 1).fits, "RT0: need %ld against the capacity", P.need);
    P = hi(5, 256, 4, 2, BIG);                                   // Np = PC = 1280, NPp = 5120
    CHECK(P.PC == 1280 && P.NPp == 5120 && P.fits, "NPp = 5120: PC %ld NPp %ld fits %d", P.PC, P.NPp, (int)P.fits);
    CHECK(P.need == 64 + 16 + 176 + 3 * 5120L + 4 * 1280L + 3 * (256 + 6), "NPp = 5120: need %ld", P.need);
    P = hi(5, 257, 4, 2, BIG);                                   // Np = 1285: the next pitch
    CHECK(P.PC == 1344 && P.NPp == 5376 && !P.fits, "NPp = 5376: PC %ld NPp %ld fits %d", P.PC, P.NPp, (int)P.fits);
    CHECK(hi(35, 34, 4, 9, BIG).fits && !hi(35, 34, 4, 10, BIG).fits, "nine modes at the most");
    CHECK(hi(7, 6, 27, 9, BIG).fits && !hi(7, 6, 28, 9, BIG).fits, "27 moments at the most");
    P = hi(35, 34, 4, 2, BIG);
    CHECK(hi(35, 34, 4, 2, P.need).fits && !hi(35, 34, 4, 2, P.need - 1).fits, "bubbles: need %ld against the capacity", P.need);
}

int main()
{
    struct Shape { int nx, ny, nz, nm; };
    const Shape shapes[] = { { 4, 8, 8, 1 }, { 9, 8, 3, 1 }, { 12, 11, 10, 1 }, { 250, 1, 1, 1 }, { 47, 45, 1, 1 }, { 5, 3, 1, 1 }, { 38, 38, 1, 1 },
                             { 6, 3, 2, 4 }, { 21, 5, 1, 3 }, { 9, 8, 7, 4 }, { 5, 3, 1, 2 }, { 34, 34, 1, 3 } };
    int cases = 0;
    for (const Shape &s : shapes)
        for (int two = 0; two <= 1; ++two) { slots(s.nx, s.ny, s.nz, s.nm, two != 0); ++cases; }
    {   // (9,8,7) with four modes has more slots than the workgroup has threads
        const long nl[3] = { 56, 63, 72 };
        if (lane_plan(3, 9, 8, 7, nl, 1, 8, 4, true, BIG).slot0[3] <= 512) { ++failures; fprintf(stderr, "FAIL 9x8x7 with 4 modes has no more than 512 slots\n"); }
    }
    plan_edges();
    if (!failures) printf("ok   %d meshes\n", cases);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
