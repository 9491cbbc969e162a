// The runtime options of a handle (nf_set_option / nf_get_option): every key is declared here once -- its field and default in NfOptions,
// and in nf_option_rows() (or nf_option_rows_more()) its normaliser, which twins take it (team_copy_options) and what setting it invalidates.  Plain C++: no device
// code, so that it can be built and run on its own (tests/host/options_main.cpp).
#pragma once
#include <climits>
#include <cstring>
#include <string>

constexpr long NF_OPT_RED_GRID = 1024;   // RED_GRID of neutfem_hip.hip (asserted equal there): default and cap of the reduction-shaped grids

// One field per key, named as the key.  Everything is long: one member-pointer type serves the whole table.
struct NfOptions {
    // small slabs (a rank's share at strong-scaling sizes): a pass on 2 M cells does not fill the chip, so the y pass runs BESIDE the x
    // pass on a stream of its own, into its own vector; the accumulation pass of the z lines adds the two (SlabArgs::yadd)
    long xy_overlap = 1, xy_overlap_max_cells = 6L << 20;
    // the interface planes travel on a communicator of their own (created collectively in team_prepare), so that the first contact with
    // RCCL on several GPUs can A/B "one communicator driven from two streams" against "one communicator per stream"
    long xchg_comm = 0;
    // single-reduction CG on slab teams (Cg1 in nf_kernels.h): one all-reduce per CG iteration instead of two
    // -1 (default): slabs of at most cg_single_reduce_max_cells cells on every rank (the largest slab of the TEAM decides, all-reduced in team_prepare).
    // With the chain-solve endpoint pass the form cost 4 us per rank and iteration at 2 M cells per slab and 40 us at 16.8 M -- more than an all-reduce --
    // and was limited to small slabs; with the weighted-sum endpoint pass (k_endpoint_w) it is FASTER than the two-reduction route in device time alone
    // at every size measured (256^3 as 2 / 4 / 8 slabs: -6.5 / -7.9 / -5.5 %, 512^3 as 8: -3.2 %; profiles/r04_d_*), so the limit is out of the way.
    long cg_single_reduce = -1, cg_single_reduce_max_cells = 1L << 40;
    long endpoint_weights = 1;      // its endpoint pass as two weighted sums per line (k_endpoint_w) instead of a chain solve
    // Vector reduce (multi-rank, one slab per rank, equal slab shapes): the block partials of p.q and |r|^2 are all-reduced as they are
    // (a few KB: still latency-bound) and the consuming kernels sum them, every block redundantly (nf_team::d_vec)
    long vec_reduce = 1;
    long host_pub = 1;              // low-latency scalar readback (k_publish); the library clears it when the mapped page cannot be made
    long prof_every = 8;            // event-timed launches: every prof_every-th Schur apply of a profiled solve (>= 1)
    long cg_batch = 0;              // CG iterations launched between two looks at the residual: 0 = automatic (NEUTFEM_CG_BATCH presets it)
    // 192^3 (7.1 M cells): 229 -> 233 us per CG iteration with them, 224^3 (11.2 M): 389 -> 356, 256^3: 599 -> 550
    long nt_loads = 1, nt_min_cells = 8000000;   // streaming (non-temporal) loads in the y / z passes of undivided meshes larger than this
    // fused CG on an undivided RT0-P0 mesh: x_sol is updated in every M-th x pass only, from a ring of M direction buffers (nf_xsol_ring.h; M-1
    // extra vectors per solver).  1 (0) = in every pass; 2 .. 8 = that M wherever eligible; -1 = XSOL_BATCH_AUTO beyond cg_lean_max_cells, else 1
    long xsol_batch = -1;
    long cg_fuse = 1;               // x += alpha p, p = r + beta p folded into the next pass that reads p (bit-identical iterates)
    long xcd = -1;                  // each XCD gets one contiguous range of tiles: bit 0 the y passes, bit 1 the z passes; -1 = the y passes of meshes beyond nt_min_cells
    long outer_dev = 1;             // the outer loop of the diagonal-Schur path stays on the device (undivided mesh, no CMFD)
    // the consumer of a reduction derives the CG scalars itself: no finalize launches on undivided meshes of at most cg_lean_max_cells cells
    // (cg_lean_grid = blocks of the residual update, 1 .. 1024), no k_cg_logic launches on slab teams
    long cg_lean = 1, cg_lean_grid = NF_OPT_RED_GRID;
    long cg_lean_max_cells = 4L << 20;   // above that the redundant partial sums of 16 k x-pass blocks cost what the two tiny kernels cost
    long sep_fold = 1;              // slab teams form the separator values inside the accumulation pass of the z lines (no k_separators launch)
    // tuning overrides of the y/z line kernel, 0 = automatic: s_tx in {8, 16, 32, 64} columns per block (the partial-sum buffer is sized for >= 8,
    // slab_partial_need), s_seg in {4, 8, 16, 32} (the instantiated segment lengths), s_wsmin = segments per line from which whole wavefronts
    // scan the summaries, 0 .. 100000
    long s_tx = 0, s_seg = 0, s_wsmin = 0;
    long split_dot = 1;             // big undivided RT0-P0 meshes: per-pass shares of p.q (team_schur_apply): 0 never, 1 where a chunked pass runs, 2 always
    long s_long_dirs = 3;           // directions that may take the chunked kernel: bit 0 = y, bit 1 = z
    long s_long_min_y = 255;        // y lines longer than this take the chunked kernel (s_long_min: z lines); 1 .. 10^6
    // tables of distinct lines (LineDict in nf_kernels.h) for the streaming passes of undivided RT0-P0 meshes.  line_dict: -1 = the directions
    // that measurably gain (LINE_DICT_AUTO_DIRS), 0 = off, 1 = every direction whose lines qualify; line_dict_dirs: bit 0 = x, 1 = y, 2 = z;
    // line_dict_max_bytes: per group and direction, at most 2^30: 32-bit byte offsets inside the kernels (three 512 KiB tables stay below half of
    // one XCD's 4 MiB L2; not swept -- the benchmark's tables are 12 - 110 KB); line_dict_fp_bits < 128 truncates the fingerprints so that tests
    // can make them collide
    long line_dict = -1, line_dict_dirs = 7, line_dict_fp_bits = 128, line_dict_max_bytes = 512L * 1024;
    long s_long = -1, s_long_min = 256;   // chunked long-line pass (k_schur_c): -1 auto (lines longer than s_long_min), 0 off, 1 always
    long c_early = -1;              // its table-backed form: vector loads of both chunks issued up front (k_schur_c EARLY): -1 auto (C_EARLY_AUTO), 0, 1, 2
    // staged form of the table-backed y / z passes (k_schur_s SV_STAGE: persistent blocks, the next tile's x copied into LDS under the scans).
    // s_stage: -1 = the directions of S_STAGE_AUTO_DIRS where a block has a next tile to fetch, 0 = off, 1 = wherever eligible;
    // s_stage_grid: blocks of such a launch, 0 = one per compute unit (at most 2^20)
    long s_stage = -1, s_stage_grid = 0;
    long tile_full = -1;            // whole-tile form of the staged k_schur_s and the table-backed early-load k_schur_c (FULL): -1 auto (on where eligible), 0, 1
    // fused-direction CG (two launches per iteration) up to this many cells.  Measured crossover against the four-launch lean path after
    // the round-2 latency work: 64^3 19.1 vs 27.2 us per CG iteration, 80^3 39.1 vs 34.5, 128^3 77.7 vs 70.9, 160^3 221 vs 150
    long cg_fuse3 = 1, cg_fuse3_max_cells = 400000;
    long sens_grid = NF_OPT_RED_GRID;   // blocks of the nf_sensitivity launches (grid stride beyond), 1 .. 65536
    long kin_grid = NF_OPT_RED_GRID;    // blocks of k_kin_forms, at most RED_GRID (grid stride beyond)
    // whole CG solve in one launch on the workgroups of one XCD (k_cg_xcd): RT0-P0 meshes between the one-workgroup resident kernel and
    // cg_xcd_max_cells.  One XCD has an eighth of the chip's compute units and L2 (4 MiB): beyond that the launch path wins back.  The library
    // clears cg_xcd / keff_xcd on a refused one-XCD launch.  cg_xcd_id 8..15: no such XCD -- nobody registers, the solve falls back (tests)
    long cg_xcd = 1, keff_xcd = 1, cg_xcd_id = 0, cg_xcd_groups = 32, cg_xcd_min_cells = 2000, cg_xcd_max_cells = 28000;
    // whole SolveKeff in one workgroup (k_resident_keff) up to this many flux DOFs per group; setting resident_max_dofs caps both variants:
    // it also sets resident_serial_max_dofs to min(value, 5120)
    long resident = 1, resident_lds = 1, resident_serial = 1, resident_two_sided = 1, resident_max_dofs = 2500, resident_serial_max_dofs = 5120;
    // explicit-S branch with a dense S^-1 up to this many flux DOFs per group, at most 8192 (the oracle's own limit: exact on both sides over
    // the same range; 288 MB per group at 6000)
    long direct_max_dofs = 6000;
    long transient_rebalance = 1;   // kept per HANDLE (nf_solver), not per team: the table only normalises it
};

// what a changed value invalidates (nf_set_option applies all four, a copy to a twin DICT or else REGIME)
enum : unsigned {
    NF_FX_RELINK = 1,        // the separator diagonals and the counts agreed across ranks: exchange again
    NF_FX_RELINK_MULTI = 2,  // the same, on teams of several ranks only (the partial counts agreed for the vector reduce depend on the tile shape)
    NF_FX_DICT = 4,          // the tables of distinct lines were built under it: drop them
    NF_FX_REGIME = 8         // moves a mesh into or out of the streaming kernels: slabs without tables look again at the next apply (a mesh whose
                             // lines do not repeat pays the fingerprints and the host sort once per build, not once per option)
};
// which twins take a key: SOLVE = every twin (what chooses its solve), PASS = twins of the caller's mesh kind only (what the launch plans of
// an apply and the scalar readback read), NONE = stays with the handle it was set on
enum NfCopy { NF_COPY_NONE, NF_COPY_SOLVE, NF_COPY_PASS };
enum NfNorm {
    NF_BOOL,     // value != 0
    NF_CLAMP,    // into [lo, hi]
    NF_MASK,     // value & hi; lo = -1: negative values store -1
    NF_POW2,     // 0 (auto) or a power of two in [lo, hi], else the row's error
    NF_ATLEAST,  // >= lo, else the row's error
    NF_RAW,      // as given; with `also`: that field = min(value, hi)
    NF_INT,      // as given, narrowed to int
    NF_RETIRED   // accepted, no effect, reads 0
};
struct NfOptionRow { const char *key; long NfOptions::*field; NfNorm norm; long lo, hi; NfCopy copy; unsigned effects; const char *err; long NfOptions::*also; };

inline const NfOptionRow *nf_option_rows(int *n)
{
#define NF_ROW(k, ...) { #k, &NfOptions::k, __VA_ARGS__ }
    static const NfOptionRow rows[] = {
        NF_ROW(s_tx, NF_POW2, 8, 64, NF_COPY_PASS, NF_FX_RELINK_MULTI | NF_FX_REGIME, "nf_set_option: s_tx must be 0 (auto), 8, 16, 32 or 64", nullptr),
        NF_ROW(s_seg, NF_POW2, 4, 32, NF_COPY_PASS, NF_FX_RELINK_MULTI | NF_FX_REGIME, "nf_set_option: s_seg must be 0 (auto), 4, 8, 16 or 32", nullptr),
        { "s_pair", nullptr, NF_RETIRED, 0, 0, NF_COPY_NONE, 0, nullptr, nullptr },        // the two-columns-per-thread variant lost to occupancy
        { "x_two_phase", nullptr, NF_RETIRED, 0, 0, NF_COPY_NONE, 0, nullptr, nullptr },   // two load phases in the x pass inside CG: measured no gain (docs/HISTORY.md)
        NF_ROW(s_wsmin, NF_CLAMP, 0, 100000, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(vec_reduce, NF_BOOL, 0, 1, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(cg_single_reduce, NF_CLAMP, -1, 1, NF_COPY_SOLVE, NF_FX_RELINK, nullptr, nullptr),
        NF_ROW(cg_single_reduce_max_cells, NF_CLAMP, 0, LONG_MAX, NF_COPY_SOLVE, NF_FX_RELINK, nullptr, nullptr),
        NF_ROW(endpoint_weights, NF_BOOL, 0, 1, NF_COPY_SOLVE, NF_FX_RELINK, nullptr, nullptr),
        NF_ROW(xchg_comm, NF_BOOL, 0, 1, NF_COPY_NONE, NF_FX_RELINK_MULTI, nullptr, nullptr),
        NF_ROW(xy_overlap, NF_BOOL, 0, 1, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(xy_overlap_max_cells, NF_CLAMP, 0, LONG_MAX, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(split_dot, NF_CLAMP, 0, 2, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(s_long, NF_CLAMP, -1, 1, NF_COPY_PASS, NF_FX_REGIME, nullptr, nullptr),
        NF_ROW(s_long_dirs, NF_MASK, 0, 3, NF_COPY_PASS, NF_FX_REGIME, nullptr, nullptr),
        NF_ROW(s_long_min_y, NF_CLAMP, 1, 1000000, NF_COPY_PASS, NF_FX_REGIME, nullptr, nullptr),
        NF_ROW(s_long_min, NF_CLAMP, 1, 1000000, NF_COPY_PASS, NF_FX_REGIME, nullptr, nullptr),
        NF_ROW(c_early, NF_CLAMP, -1, 2, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(s_stage, NF_CLAMP, -1, 1, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(tile_full, NF_CLAMP, -1, 1, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(s_stage_grid, NF_CLAMP, 0, 1L << 20, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(line_dict, NF_CLAMP, -1, 1, NF_COPY_PASS, NF_FX_DICT, nullptr, nullptr),
        NF_ROW(line_dict_dirs, NF_MASK, 0, 7, NF_COPY_PASS, NF_FX_DICT, nullptr, nullptr),
        NF_ROW(line_dict_max_bytes, NF_CLAMP, 0, 1L << 30, NF_COPY_PASS, NF_FX_DICT, nullptr, nullptr),
        NF_ROW(line_dict_fp_bits, NF_CLAMP, 0, 128, NF_COPY_PASS, NF_FX_DICT, nullptr, nullptr),
        NF_ROW(cg_batch, NF_INT, 0, 0, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_fuse, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(xcd, NF_MASK, -1, 7, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(host_pub, NF_BOOL, 0, 1, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(prof_every, NF_ATLEAST, 1, 0, NF_COPY_PASS, 0, "prof_every must be >= 1", nullptr),
        NF_ROW(nt_loads, NF_BOOL, 0, 1, NF_COPY_PASS, NF_FX_REGIME, nullptr, nullptr),
        NF_ROW(nt_min_cells, NF_RAW, 0, 0, NF_COPY_PASS, NF_FX_REGIME, nullptr, nullptr),
        NF_ROW(outer_dev, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_lean, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(sep_fold, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_lean_max_cells, NF_RAW, 0, 0, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(resident, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(resident_lds, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(resident_serial, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(resident_two_sided, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(resident_max_dofs, NF_RAW, 0, 5120, NF_COPY_SOLVE, 0, nullptr, &NfOptions::resident_serial_max_dofs),
        NF_ROW(resident_serial_max_dofs, NF_RAW, 0, 0, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(direct_max_dofs, NF_CLAMP, 0, 8192, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_fuse3, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_xcd, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(keff_xcd, NF_BOOL, 0, 1, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_xcd_min_cells, NF_RAW, 0, 0, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_xcd_max_cells, NF_RAW, 0, 0, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_xcd_id, NF_MASK, 0, 15, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_xcd_groups, NF_CLAMP, 1, 64, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_fuse3_max_cells, NF_RAW, 0, 0, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(cg_lean_grid, NF_CLAMP, 1, 1024, NF_COPY_SOLVE, 0, nullptr, nullptr),
        NF_ROW(sens_grid, NF_CLAMP, 1, 65536, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(kin_grid, NF_CLAMP, 1, NF_OPT_RED_GRID, NF_COPY_PASS, 0, nullptr, nullptr),
        NF_ROW(transient_rebalance, NF_BOOL, 0, 1, NF_COPY_NONE, 0, nullptr, nullptr),
    };
#undef NF_ROW
    *n = (int)(sizeof rows / sizeof rows[0]);
    return rows;
}
// Rows added since tests/host/options_main.cpp wrote out the table above key by key (it counts those rows): declared the same way, found, set,
// read and copied by the same functions; tests/host/xsol_option_main.cpp writes out what they must do.
inline const NfOptionRow *nf_option_rows_more(int *n)
{
    static const NfOptionRow rows[] = {
        { "xsol_batch", &NfOptions::xsol_batch, NF_CLAMP, -1, 8, NF_COPY_SOLVE, 0, nullptr, nullptr },
    };
    *n = (int)(sizeof rows / sizeof rows[0]);
    return rows;
}
inline const NfOptionRow *nf_option_find(const char *key)
{
    int n = 0; const NfOptionRow *rows = nf_option_rows(&n);
    for (int i = 0; i < n; ++i) if (!strcmp(key, rows[i].key)) return rows + i;
    rows = nf_option_rows_more(&n);
    for (int i = 0; i < n; ++i) if (!strcmp(key, rows[i].key)) return rows + i;
    return nullptr;
}

// Stores the normalised value; *effects = what the key invalidates, whether or not the value moved.  false: *err says why, nothing stored.
inline bool nf_options_set(NfOptions &o, const char *key, long value, unsigned *effects, std::string *err)
{
    const NfOptionRow *r = nf_option_find(key);
    if (!r) { *err = std::string("nf_set_option: unknown key ") + key; return false; }
    long v = value;
    switch (r->norm) {
    case NF_BOOL: v = value != 0; break;
    case NF_CLAMP: v = value < r->lo ? r->lo : value > r->hi ? r->hi : value; break;
    case NF_MASK: v = r->lo < 0 && value < 0 ? -1 : value & r->hi; break;
    case NF_POW2: if (value != 0 && (value < r->lo || value > r->hi || (value & (value - 1)))) { *err = r->err; return false; } break;
    case NF_ATLEAST: if (value < r->lo) { *err = r->err; return false; } break;
    case NF_RAW: if (r->also) o.*r->also = value < r->hi ? value : r->hi; break;
    case NF_INT: v = (int)value; break;
    case NF_RETIRED: break;
    }
    if (r->field) o.*r->field = v;
    *effects = r->effects;
    return true;
}
// The stored value; retired keys read 0.  false: no such key.
inline bool nf_options_get(const NfOptions &o, const char *key, long *value)
{
    const NfOptionRow *r = nf_option_find(key);
    if (!r) return false;
    *value = r->field ? o.*r->field : 0;
    return true;
}
// dst takes the SOLVE keys of src and, for a twin of the same mesh kind, the PASS keys.  Returns the DICT / REGIME effects of the keys whose
// value changed: the twin's link state is its own, a copy never asks for RELINK.
inline unsigned nf_options_copy(NfOptions &dst, const NfOptions &src, bool same_mesh_kind)
{
    unsigned fx = 0;
    for (int part = 0; part < 2; ++part) {
        int n = 0; const NfOptionRow *rows = part ? nf_option_rows_more(&n) : nf_option_rows(&n);
        for (int i = 0; i < n; ++i) {
            const NfOptionRow &r = rows[i];
            if (r.copy == NF_COPY_NONE || (r.copy == NF_COPY_PASS && !same_mesh_kind) || dst.*r.field == src.*r.field) continue;
            dst.*r.field = src.*r.field; fx |= r.effects;
        }
    }
    return fx & (NF_FX_DICT | NF_FX_REGIME);
}
