// Stand-alone check of the fingerprint grouping behind the tables of distinct lines (neutfem_amd/csrc/nf_line_groups.h): hand-made
// fingerprint lists, no device.  Meant to be built with -fsanitize=address,undefined as well as plainly; exits non-zero on a mismatch.
#include "../../neutfem_amd/csrc/nf_line_groups.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
static void expect(const char *what, const std::vector<nf_fp128> &fp, int want_n, const std::vector<int> &want_ids, const std::vector<int> &want_reps)
{
    std::vector<int> ids(3, 77), reps(5, 99);                     // stale contents must not survive
    const int n = nf_group_lines(fp.data(), (long)fp.size(), ids, reps);
    if (n != want_n || ids != want_ids || reps != want_reps) {
        ++failures;
        fprintf(stderr, "FAIL %s: %d groups (want %d), ids", what, n, want_n);
        for (int v : ids) fprintf(stderr, " %d", v);
        fprintf(stderr, ", reps");
        for (int v : reps) fprintf(stderr, " %d", v);
        fprintf(stderr, "\n");
    } else printf("ok   %s\n", what);
}

int main()
{
    const nf_fp128 A = { 1, 2 }, B = { 1, 3 }, C = { 0, 2 }, D = { ~0ull, ~0ull };
    expect("no lines", {}, 0, {}, {});
    expect("one line", { A }, 1, { 0 }, { 0 });
    expect("all equal", { A, A, A, A, A }, 1, { 0, 0, 0, 0, 0 }, { 0 });
    expect("all distinct", { D, C, B, A }, 4, { 0, 1, 2, 3 }, { 0, 1, 2, 3 });                 // numbered by line, not by fingerprint value
    expect("repeats", { B, A, B, C, A, B, D, C }, 4, { 0, 1, 0, 2, 1, 0, 3, 2 }, { 0, 1, 3, 6 });
    expect("differ in lo only", { { 5, 9 }, { 6, 9 }, { 5, 9 } }, 2, { 0, 1, 0 }, { 0, 1 });
    expect("differ in hi only", { { 5, 9 }, { 5, 8 }, { 5, 8 } }, 2, { 0, 1, 1 }, { 0, 1 });
    // truncated fingerprints (line_dict_fp_bits): lines that differ collide into one group; grouping cannot know, the device-side verification does
    expect("collisions", { { 3, 0 }, { 3, 0 }, { 1, 0 }, { 3, 0 } }, 2, { 0, 0, 1, 0 }, { 0, 2 });
    {   // many lines, few values: representatives are the first occurrences
        std::vector<nf_fp128> fp; std::vector<int> ids, reps;
        unsigned s = 12345u;
        for (int i = 0; i < 65536; ++i) { s = s * 1664525u + 1013904223u; fp.push_back({ (s >> 16) % 12u, 7 }); }
        const int n = nf_group_lines(fp.data(), (long)fp.size(), ids, reps);
        bool ok = n == 12 && (int)reps.size() == 12;
        for (int i = 0; ok && i < 65536; ++i) ok = fp[(size_t)reps[(size_t)ids[(size_t)i]]].lo == fp[(size_t)i].lo && reps[(size_t)ids[(size_t)i]] <= i;
        for (int r = 1; ok && r < n; ++r) ok = reps[(size_t)r - 1] < reps[(size_t)r];
        if (!ok) { ++failures; fprintf(stderr, "FAIL 65536 lines of 12 kinds\n"); } else printf("ok   65536 lines of 12 kinds\n");
    }
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
