// Stand-alone check of the option "xsol_batch" (neutfem_amd/csrc/nf_options.h): its default, normaliser, effects and copy class written
// out by hand, as tests/host/options_main.cpp does for the keys of the table; plain C++, no device.  Meant to be built with
// -fsanitize=address,undefined as well as plainly; exits non-zero on a mismatch.
#include "../../neutfem_amd/csrc/nf_options.h"

#include <cstdio>
#include <cstdlib>
#include <set>

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; fprintf(stderr, "FAIL "); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

int main()
{
    const long in[] = { -7, -1, 0, 1, 2, 3, 5, 8, 64, 100, 4096, 10000000L, 1L << 40 };
    const long want[] = { -1, -1, 0, 1, 2, 3, 5, 8, 8, 8, 8, 8, 8 };
    long v = 99;
    {   // declared once: found by name, in neither list twice
        int n = 0, m = 0; const NfOptionRow *rows = nf_option_rows(&n), *more = nf_option_rows_more(&m);
        std::set<std::string> keys;
        for (int i = 0; i < n; ++i) keys.insert(rows[i].key);
        for (int i = 0; i < m; ++i) keys.insert(more[i].key);
        CHECK((int)keys.size() == n + m && keys.count("xsol_batch") == 1, "%d + %d rows, %zu distinct keys", n, m, keys.size());
        for (int i = 0; i < m; ++i) CHECK(more[i].field && nf_option_find(more[i].key) == more + i, "row %s is not found", more[i].key);
        if (!failures) printf("ok   declared once\n");
    }
    {
        const int f0 = failures;
        const NfOptions fresh;
        CHECK(nf_options_get(fresh, "xsol_batch", &v) && v == -1 && fresh.xsol_batch == -1, "default %ld", v);
        for (int i = 0; i < 13; ++i) {
            NfOptions o; unsigned fx = 99; std::string err;
            CHECK(nf_options_set(o, "xsol_batch", in[i], &fx, &err) && fx == 0, "xsol_batch = %ld refused or effects %u", in[i], fx);
            CHECK(nf_options_get(o, "xsol_batch", &v) && v == want[i] && o.xsol_batch == want[i], "xsol_batch = %ld stored %ld, want %ld", in[i], v, want[i]);
            o.xsol_batch = fresh.xsol_batch;
            CHECK(o.cg_fuse == fresh.cg_fuse && o.xcd == fresh.xcd && o.cg_batch == fresh.cg_batch, "xsol_batch = %ld touched another field", in[i]);
        }
        if (failures == f0) printf("ok   default, normaliser, effects\n");
    }
    {   // what chooses a solve goes to every twin, whatever its mesh kind; the copy asks for nothing
        const int f0 = failures;
        for (int kind = 0; kind < 2; ++kind) {
            NfOptions src, dst; src.xsol_batch = 4;
            unsigned fx = nf_options_copy(dst, src, kind == 1);
            CHECK(dst.xsol_batch == 4 && fx == 0, "copy (same kind %d): %ld, effects %u", kind, dst.xsol_batch, fx);
            fx = nf_options_copy(dst, src, kind == 1);
            CHECK(dst.xsol_batch == 4 && fx == 0, "second copy (same kind %d)", kind);
        }
        if (failures == f0) printf("ok   copy\n");
    }
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
