// Stand-alone check of the option table (neutfem_amd/csrc/nf_options.h): every key's normaliser, default, effects and copy class against
// values written out here by hand from the documented behaviour of nf_set_option -- never computed from the table itself.  No device.
// Meant to be built with -fsanitize=address,undefined as well as plainly; exits non-zero on a mismatch.
#include "../../neutfem_amd/csrc/nf_options.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <set>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAIL " __VA_ARGS__); fputc('\n', stderr); } } while (0)

static const int NIN = 13;
static const long INPUTS[NIN] = { -7, -1, 0, 1, 2, 3, 5, 8, 64, 100, 4096, 10000000L, 1L << 40 };
static const long E = LONG_MIN;                                   // the set is refused (NF_ERR_ARG)
enum Cls { N, S, P };                                             // NONE, SOLVE (every twin), PASS (twins of the same mesh kind)
static const unsigned RELINK = 1, RELINK_MULTI = 2, DICT = 4, REGIME = 8;
// key, default, effects (RELINK 1, RELINK_MULTI 2, DICT 4, REGIME 8), copy class, retired, stored value per input
struct Want { const char *key; long dflt; unsigned fx; Cls cls; int retired; long v[NIN]; };
static const Want WANT[] = {
    { "c_early", -1L, 0, P, 0, { -1L, -1L, 0L, 1L, 2L, 2L, 2L, 2L, 2L, 2L, 2L, 2L, 2L } },
    { "cg_batch", 0L, 0, S, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 0L } },
    { "cg_fuse", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "cg_fuse3", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "cg_fuse3_max_cells", 400000L, 0, S, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "cg_lean", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "cg_lean_grid", 1024L, 0, S, 0, { 1L, 1L, 1L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 1024L, 1024L, 1024L } },
    { "cg_lean_max_cells", 4194304L, 0, S, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "cg_single_reduce", -1L, 1, S, 0, { -1L, -1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "cg_single_reduce_max_cells", 1099511627776L, 1, S, 0, { 0L, 0L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "cg_xcd", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "cg_xcd_groups", 32L, 0, S, 0, { 1L, 1L, 1L, 1L, 2L, 3L, 5L, 8L, 64L, 64L, 64L, 64L, 64L } },
    { "cg_xcd_id", 0L, 0, S, 0, { 9L, 15L, 0L, 1L, 2L, 3L, 5L, 8L, 0L, 4L, 0L, 0L, 0L } },
    { "cg_xcd_max_cells", 28000L, 0, S, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "cg_xcd_min_cells", 2000L, 0, S, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "direct_max_dofs", 6000L, 0, S, 0, { 0L, 0L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 8192L, 8192L } },
    { "endpoint_weights", 1L, 1, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "host_pub", 1L, 0, P, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "keff_xcd", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "kin_grid", 1024L, 0, P, 0, { 1L, 1L, 1L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 1024L, 1024L, 1024L } },
    { "line_dict", -1L, 4, P, 0, { -1L, -1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "line_dict_dirs", 7L, 4, P, 0, { 1L, 7L, 0L, 1L, 2L, 3L, 5L, 0L, 0L, 4L, 0L, 0L, 0L } },
    { "line_dict_fp_bits", 128L, 4, P, 0, { 0L, 0L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 128L, 128L, 128L } },
    { "line_dict_max_bytes", 524288L, 4, P, 0, { 0L, 0L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1073741824L } },
    { "nt_loads", 1L, 8, P, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "nt_min_cells", 8000000L, 8, P, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "outer_dev", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "prof_every", 8L, 0, P, 0, { E, E, E, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "resident", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "resident_lds", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "resident_max_dofs", 2500L, 0, S, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "resident_serial", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "resident_serial_max_dofs", 5120L, 0, S, 0, { -7L, -1L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
    { "resident_two_sided", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "s_long", -1L, 8, P, 0, { -1L, -1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "s_long_dirs", 3L, 8, P, 0, { 1L, 3L, 0L, 1L, 2L, 3L, 1L, 0L, 0L, 0L, 0L, 0L, 0L } },
    { "s_long_min", 256L, 8, P, 0, { 1L, 1L, 1L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 1000000L, 1000000L } },
    { "s_long_min_y", 255L, 8, P, 0, { 1L, 1L, 1L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 1000000L, 1000000L } },
    { "s_pair", 0L, 0, N, 1, { 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L } },
    { "s_seg", 0L, 10, P, 0, { E, E, 0L, E, E, E, E, 8L, E, E, E, E, E } },
    { "s_stage", -1L, 0, P, 0, { -1L, -1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "s_stage_grid", 0L, 0, P, 0, { 0L, 0L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 1048576L, 1048576L } },
    { "s_tx", 0L, 10, P, 0, { E, E, 0L, E, E, E, E, 8L, 64L, E, E, E, E } },
    { "s_wsmin", 0L, 0, P, 0, { 0L, 0L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 100000L, 100000L } },
    { "sens_grid", 1024L, 0, P, 0, { 1L, 1L, 1L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 65536L, 65536L } },
    { "sep_fold", 1L, 0, S, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "split_dot", 1L, 0, P, 0, { 0L, 0L, 0L, 1L, 2L, 2L, 2L, 2L, 2L, 2L, 2L, 2L, 2L } },
    { "tile_full", -1L, 0, P, 0, { -1L, -1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "transient_rebalance", 1L, 0, N, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "vec_reduce", 1L, 0, P, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "x_two_phase", 0L, 0, N, 1, { 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L } },
    { "xcd", -1L, 0, P, 0, { -1L, -1L, 0L, 1L, 2L, 3L, 5L, 0L, 0L, 4L, 0L, 0L, 0L } },
    { "xchg_comm", 0L, 2, N, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "xy_overlap", 1L, 0, P, 0, { 1L, 1L, 0L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L, 1L } },
    { "xy_overlap_max_cells", 6291456L, 0, P, 0, { 0L, 0L, 0L, 1L, 2L, 3L, 5L, 8L, 64L, 100L, 4096L, 10000000L, 1099511627776L } },
};
static const int NWANT = (int)(sizeof WANT / sizeof WANT[0]);

static bool same(const NfOptions &a, const NfOptions &b) { return !memcmp(&a, &b, sizeof a); }   // all long: no padding
static long get(const NfOptions &o, const char *key) { long v = E; if (!nf_options_get(o, key, &v)) { ++failures; fprintf(stderr, "FAIL get %s\n", key); } return v; }

int main()
{
    const NfOptions fresh;
    {   // the table: 55 keys, none twice, each one expected here
        int n = 0; const NfOptionRow *rows = nf_option_rows(&n);
        std::set<std::string> keys; for (int i = 0; i < n; ++i) keys.insert(rows[i].key);
        CHECK(n == 55 && keys.size() == 55 && NWANT == 55, "table has %d rows, %zu distinct, %d expected here", n, keys.size(), NWANT);
        for (const Want &w : WANT) CHECK(keys.count(w.key) == 1, "key %s is not in the table", w.key);
        if (!failures) printf("ok   55 keys, no duplicates\n");
    }
    {   // defaults
        const int f0 = failures;
        for (const Want &w : WANT) CHECK(get(fresh, w.key) == w.dflt, "default of %s: %ld, want %ld", w.key, get(fresh, w.key), w.dflt);
        CHECK(fresh.s_tx == 0 && fresh.cg_single_reduce_max_cells == (1L << 40) && fresh.line_dict_max_bytes == 524288 && fresh.kin_grid == 1024, "defaults read from the fields");
        if (failures == f0) printf("ok   defaults\n");
    }
    {   // every key, every input: stored value or refusal, effects
        const int f0 = failures;
        for (const Want &w : WANT) for (int i = 0; i < NIN; ++i) {
            NfOptions o; unsigned fx = 99; std::string err;
            const bool ok = nf_options_set(o, w.key, INPUTS[i], &fx, &err);
            if (w.v[i] == E) { CHECK(!ok && !err.empty() && same(o, fresh), "%s = %ld: accepted or stored (%s)", w.key, INPUTS[i], err.c_str()); continue; }
            CHECK(ok && err.empty(), "%s = %ld refused: %s", w.key, INPUTS[i], err.c_str());
            CHECK(get(o, w.key) == w.v[i], "%s = %ld stored %ld, want %ld", w.key, INPUTS[i], get(o, w.key), w.v[i]);
            CHECK(fx == w.fx, "%s = %ld: effects %u, want %u", w.key, INPUTS[i], fx, w.fx);
            if (w.retired) CHECK(same(o, fresh), "retired key %s = %ld changed the options", w.key, INPUTS[i]);
            // nothing but the key's own field moves (resident_max_dofs moves two)
            if (!w.retired && strcmp(w.key, "resident_max_dofs"))
                for (const Want &u : WANT) if (strcmp(u.key, w.key)) CHECK(get(o, u.key) == u.dflt, "%s = %ld moved %s", w.key, INPUTS[i], u.key);
        }
        if (failures == f0) printf("ok   normalisers and effects\n");
    }
    {   // the refusals carry these texts
        const int f0 = failures;
        NfOptions o; unsigned fx; std::string err;
        CHECK(!nf_options_set(o, "s_tx", 5, &fx, &err) && err == "nf_set_option: s_tx must be 0 (auto), 8, 16, 32 or 64", "s_tx message: %s", err.c_str());
        CHECK(!nf_options_set(o, "s_seg", 64, &fx, &err) && err == "nf_set_option: s_seg must be 0 (auto), 4, 8, 16 or 32", "s_seg message: %s", err.c_str());
        CHECK(!nf_options_set(o, "prof_every", 0, &fx, &err) && err == "prof_every must be >= 1", "prof_every message: %s", err.c_str());
        CHECK(!nf_options_set(o, "bogus", 1, &fx, &err) && err == "nf_set_option: unknown key bogus", "unknown key message: %s", err.c_str());
        long v = 5; CHECK(!nf_options_get(o, "bogus", &v) && v == 5, "get of an unknown key");
        CHECK(same(o, fresh), "a refused set stored something");
        CHECK(nf_options_set(o, "s_tx", 16, &fx, &err) && o.s_tx == 16 && nf_options_set(o, "s_seg", 4, &fx, &err) && o.s_seg == 4, "s_tx / s_seg fields");
        if (failures == f0) printf("ok   refusals\n");
    }
    {   // resident_max_dofs caps both variants
        const int f0 = failures;
        NfOptions o; unsigned fx; std::string err;
        CHECK(nf_options_set(o, "resident_max_dofs", 100, &fx, &err) && o.resident_max_dofs == 100 && o.resident_serial_max_dofs == 100, "resident_max_dofs 100");
        CHECK(nf_options_set(o, "resident_max_dofs", 10000000L, &fx, &err) && o.resident_max_dofs == 10000000L && o.resident_serial_max_dofs == 5120, "resident_max_dofs 10^7");
        CHECK(nf_options_set(o, "resident_max_dofs", -7, &fx, &err) && o.resident_max_dofs == -7 && o.resident_serial_max_dofs == -7, "resident_max_dofs -7");
        CHECK(nf_options_set(o, "resident_serial_max_dofs", 4096, &fx, &err) && o.resident_max_dofs == -7 && o.resident_serial_max_dofs == 4096, "resident_serial_max_dofs alone");
        if (failures == f0) printf("ok   resident_max_dofs moves both fields\n");
    }
    // copies: src differs from dst in every field
    NfOptions src;
    {
        long NfOptions::*f; int n = 0; const NfOptionRow *rows = nf_option_rows(&n);
        for (int i = 0; i < n; ++i) if ((f = rows[i].field)) src.*f += 1000 + i;
        for (const Want &w : WANT) if (!w.retired) CHECK(get(src, w.key) != w.dflt, "src does not differ in %s", w.key);
    }
    for (int kind = 0; kind < 2; ++kind) {
        const int f0 = failures;
        NfOptions dst; const unsigned fx = nf_options_copy(dst, src, kind == 1);
        for (const Want &w : WANT) {
            const bool moves = w.cls == S || (w.cls == P && kind == 1);
            CHECK(get(dst, w.key) == (moves ? get(src, w.key) : w.dflt), "copy (same kind %d): %s %s", kind, w.key, moves ? "stayed" : "moved");
        }
        CHECK(fx == (kind ? DICT | REGIME : 0u), "copy (same kind %d) of everything: effects %u", kind, fx);
        if (failures == f0) printf("ok   copy, same mesh kind %d\n", kind);
    }
    {   // copy effects: DICT iff a line_dict* value differed, else REGIME iff one of its eight keys differed; RELINK never
        const int f0 = failures;
        for (const Want &w : WANT) {
            if (w.retired) continue;
            NfOptions one, dst; unsigned f1; std::string err;
            const long other = !strcmp(w.key, "s_tx") ? 16 : !strcmp(w.key, "s_seg") ? 8 : w.dflt == 1 ? 0 : 1;    // legal and not the default
            CHECK(nf_options_set(one, w.key, other, &f1, &err) && get(one, w.key) != w.dflt, "%s = %ld is no change", w.key, other);
            const unsigned want_same = w.cls == N ? 0u : (w.fx & DICT) ? DICT : (w.fx & REGIME), want_other = w.cls == S ? want_same : 0u;
            unsigned fx = nf_options_copy(dst, one, true);
            CHECK(fx == want_same, "copy of a changed %s to a twin of the same kind: effects %u, want %u", w.key, fx, want_same);
            fx = nf_options_copy(dst, one, true);
            CHECK(fx == 0, "second copy of %s: effects %u although nothing changed", w.key, fx);
            NfOptions d2; fx = nf_options_copy(d2, one, false);
            CHECK(fx == want_other, "copy of a changed %s to a coarse twin: effects %u, want %u", w.key, fx, want_other);
        }
        NfOptions both, dst; unsigned f1; std::string err;
        nf_options_set(both, "line_dict_fp_bits", 64, &f1, &err); nf_options_set(both, "s_long_min", 100, &f1, &err); nf_options_set(both, "cg_single_reduce", 1, &f1, &err);
        const unsigned fx = nf_options_copy(dst, both, true);
        CHECK((fx & DICT) && !(fx & (RELINK | RELINK_MULTI)), "a table key and a regime key changed: effects %u", fx);
        CHECK(nf_options_copy(dst, fresh, true) == (DICT | REGIME) && same(dst, fresh), "copying the defaults back");
        if (failures == f0) printf("ok   copy effects\n");
    }
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
