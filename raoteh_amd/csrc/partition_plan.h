// Host planner of a partitioned batch (rt_sites_create_partitioned): the resident order of the
// sites when site i is evaluated under rate set site_set[i].  Plain C++, no HIP: the library
// exports it as rt_partition_plan, and a stand-alone program can include it on its own.
//
// A granule is G consecutive resident sites that share one copy of the transition tables in the
// pruning kernel that will run: 16 (one site tile) in the matrix-pipe layout, the workgroup's
// span of sites in the lane layout.  The plan makes every granule homogeneous in its set:
//   - a stable counting sort of the sites by set: set k's sites, in caller order, form run k;
//   - every run is padded up to a multiple of G; a pad slot repeats the LAST real site of its
//     run, so it carries valid observations (no spurious zero-probability status) and costs
//     nothing but its arithmetic; an empty set has an empty run (no granule at all).
// Outputs (slot = position in the resident order, padded = number of slots):
//   order[padded]         source site of every slot
//   slot_of_site[nsites]  the slot that holds site i itself (never a pad)
//   is_pad[padded]        1 for a pad slot
//   granule_set[padded/G] the set of every granule
//   run_begin[K + 1]      run k is the slots [run_begin[k], run_begin[k + 1])
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

struct rt_partition_layout {
    int64_t nsites = 0, K = 0, G = 0, padded = 0;
    std::vector<int64_t> order, slot_of_site, run_begin;
    std::vector<uint8_t> is_pad;
    std::vector<int32_t> granule_set;
};

// 0, or -1 (RT_ERR_INVALID): a null / non-positive argument (*bad_site = -1) or a set index
// outside 0 .. K-1 (*bad_site = the first such site); `out` is left empty then
inline int rt_partition_plan_build(const int32_t *site_set, int64_t nsites, int64_t K, int64_t G,
                                   rt_partition_layout *out, int64_t *bad_site)
{
    if (bad_site) *bad_site = -1;
    if (!out) return -1;
    *out = rt_partition_layout();
    if (!site_set || nsites < 1 || K < 1 || G < 1) return -1;
    std::vector<int64_t> count((size_t)K, 0);
    for (int64_t i = 0; i < nsites; ++i) {
        const int32_t k = site_set[i];
        if (k < 0 || (int64_t)k >= K) {
            if (bad_site) *bad_site = i;
            return -1;
        }
        count[(size_t)k] += 1;
    }
    out->nsites = nsites;
    out->K = K;
    out->G = G;
    out->run_begin.assign((size_t)K + 1, 0);
    for (int64_t k = 0; k < K; ++k)
        out->run_begin[(size_t)k + 1] = out->run_begin[(size_t)k] + (count[(size_t)k] + G - 1) / G * G;
    const int64_t padded = out->run_begin[(size_t)K];
    out->padded = padded;
    out->order.assign((size_t)padded, 0);
    out->is_pad.assign((size_t)padded, 0);
    out->slot_of_site.assign((size_t)nsites, 0);
    out->granule_set.assign((size_t)(padded / G), 0);
    // stable: the sites of a set keep their caller order
    std::vector<int64_t> next(out->run_begin.begin(), out->run_begin.end() - 1);
    for (int64_t i = 0; i < nsites; ++i) {
        const int64_t slot = next[(size_t)site_set[i]]++;
        out->order[(size_t)slot] = i;
        out->slot_of_site[(size_t)i] = slot;
    }
    for (int64_t k = 0; k < K; ++k) {
        const int64_t end = out->run_begin[(size_t)k + 1];
        // (a run with pads has at least one real site: next[k] > run_begin[k])
        for (int64_t slot = next[(size_t)k]; slot < end; ++slot) {
            out->order[(size_t)slot] = out->order[(size_t)next[(size_t)k] - 1];
            out->is_pad[(size_t)slot] = 1;
        }
        for (int64_t g = out->run_begin[(size_t)k] / G; g < end / G; ++g)
            out->granule_set[(size_t)g] = (int32_t)k;
    }
    return 0;
}
