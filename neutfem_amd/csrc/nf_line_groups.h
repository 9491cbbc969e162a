// Grouping of line fingerprints (tables of distinct lines, see LineDict in nf_kernels.h).  Plain C++: no device code, so that it can
// be built and run on its own (tests/host/line_groups_main.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct nf_fp128 { uint64_t lo, hi; };

// Lines with equal fingerprints form a group; its representative is its lowest line index.  ids[i] = the group of line i, groups numbered by
// rising representative; reps[id] = that representative.  Returns the number of groups (0 for no lines).
inline int nf_group_lines(const nf_fp128 *fp, long n, std::vector<int> &ids, std::vector<int> &reps)
{
    ids.assign((size_t)(n > 0 ? n : 0), 0); reps.clear();
    if (n <= 0) return 0;
    std::vector<int> order((size_t)n);
    for (long i = 0; i < n; ++i) order[(size_t)i] = (int)i;
    std::sort(order.begin(), order.end(), [fp](int a, int b) {
        if (fp[a].hi != fp[b].hi) return fp[a].hi < fp[b].hi;
        if (fp[a].lo != fp[b].lo) return fp[a].lo < fp[b].lo;
        return a < b;                                             // the lowest line of a group comes first
    });
    for (long i = 0; i < n; ++i) {
        const int a = order[(size_t)i];
        if (i == 0 || fp[a].hi != fp[order[(size_t)i - 1]].hi || fp[a].lo != fp[order[(size_t)i - 1]].lo) reps.push_back(a);
        ids[(size_t)a] = reps.back();                             // the representative for now, its rank below
    }
    std::sort(reps.begin(), reps.end());
    for (long i = 0; i < n; ++i) ids[(size_t)i] = (int)(std::lower_bound(reps.begin(), reps.end(), ids[(size_t)i]) - reps.begin());
    return (int)reps.size();
}
