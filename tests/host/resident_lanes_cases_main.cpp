// The plan of the resident solve's line-per-lane variants (neutfem_amd/csrc/nf_resident_lanes.h) for meshes given on the command line:
//   resident_lanes_cases CAP  DIM NX NY NZ NB NLOC NMODES  [DIM NX ...]
// CAP = the LDS a workgroup may have, in doubles.  Prints one line per mesh and per two_sided = 1 / 0:
//   fits tw[0] tw[1] tw[2] slots PC NPp need
// so that a test can check its own case table against the arithmetic the library runs (tests/test_apply_exact.py).  No device.
#include "../../neutfem_amd/csrc/nf_resident_lanes.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 2 || (argc - 2) % 7 != 0) { fprintf(stderr, "usage: %s CAP (DIM NX NY NZ NB NLOC NMODES)...\n", argv[0]); return EXIT_FAILURE; }
    const long cap = atol(argv[1]);
    for (int a = 2; a < argc; a += 7) {
        const int dim = atoi(argv[a]), nx = atoi(argv[a + 1]), ny = atoi(argv[a + 2]), nz = atoi(argv[a + 3]);
        const int nb = atoi(argv[a + 4]), nloc = atoi(argv[a + 5]), nmodes = atoi(argv[a + 6]);
        if (dim < 1 || dim > 3 || nx < 1 || ny < 1 || nz < 1) { fprintf(stderr, "bad mesh\n"); return EXIT_FAILURE; }
        const long nlines[3] = { (long)ny * nz, (long)nx * nz, (long)nx * ny };   // as nf_create fills them
        for (int two = 1; two >= 0; --two) {
            const LanePlan P = lane_plan(dim, nx, ny, nz, nlines, nb, nloc, nmodes, two != 0, cap);
            printf("%d %d %d %d %d %ld %ld %ld\n", (int)P.fits, P.tw[0], P.tw[1], P.tw[2], P.slot0[3], P.PC, P.NPp, P.need);
        }
    }
    return EXIT_SUCCESS;
}
