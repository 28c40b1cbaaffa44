// Internal, host only (no HIP): the index tables the region layer builds before a launch. A CSR segment table by
// counting sort (catchment, routing-group and ensemble segments), and the tables of a river network (routing.hip,
// routing_members.hip). tools/host_tables_check.cpp runs both under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace shyft_hip_impl {

// Counting sort of (key, item) pairs into off[n_keys + 1] / items: the items of key k are items[off[k] .. off[k + 1]),
// in the order they were enumerated (the segment sums add in that order). `pairs(emit)` calls emit(key, item) for
// every pair and runs twice, to count and to place, so it must enumerate the same pairs both times; a pair it does
// not emit is left out. Keys lie in [0, n_keys): the enumeration checks (and may throw) before it emits. Returns
// whether items is the identity 0, 1, 2, ... of its own length.
template <class Off, class Pairs>
bool build_csr(size_t n_keys, std::vector<Off>& off, std::vector<int32_t>& items, Pairs&& pairs) {
    off.assign(n_keys + 1, 0);
    pairs([&](size_t key, int32_t) { off[key + 1]++; });
    for (size_t k = 0; k < n_keys; ++k) off[k + 1] += off[k];
    items.resize(size_t(off[n_keys]));
    std::vector<Off> pos(off.begin(), off.end() - 1);
    pairs([&](size_t key, int32_t item) { items[size_t(pos[key]++)] = item; });
    for (size_t i = 0; i < items.size(); ++i)
        if (items[i] != int32_t(i)) return false;
    return true;
}

// routing::river_network as tables (core/routing.h:239-421) for P members that share the rivers: member m owns the
// group rows [group_row[m], group_row[m + 1]).
template <class Off>
struct river_tables {
    std::vector<Off> pair_off;         // [P*R + 1] CSR of the group rows of (member, river), ascending row
    std::vector<int32_t> pair_groups;  // [G]
    std::vector<int32_t> up_off, ups;  // [R + 1] CSR of the upstream rivers, ascending index (= ascending id)
    std::vector<int32_t> lvl_off, lvl_rivers;  // rivers by network level, upstream levels first, ascending index
    int n_levels() const { return int(lvl_off.size()) - 1; }
};

// The caller has checked group_river[g] in [0, R) and river_downstream[r] < R; a negative downstream is an outlet.
// Returns false when the network has a cycle (lvl_off / lvl_rivers are then not built): the caller raises its text.
template <class Off>
bool build_river_tables(size_t P, const int64_t* group_row, const int32_t* group_river, size_t R,
                        const int32_t* river_downstream, river_tables<Off>& tb) {
    build_csr(P * R, tb.pair_off, tb.pair_groups, [&](auto&& emit) {
        for (size_t m = 0; m < P; ++m)
            for (int64_t g = group_row[m]; g < group_row[m + 1]; ++g) emit(m * R + size_t(group_river[g]), int32_t(g));
    });
    build_csr(R, tb.up_off, tb.ups, [&](auto&& emit) {
        for (size_t u = 0; u < R; ++u)
            if (river_downstream[u] >= 0) emit(size_t(river_downstream[u]), int32_t(u));
    });
    // network levels: level(r) = 1 + max level of its upstream rivers (sources are level 0)
    std::vector<int32_t> level(R, -1);
    for (size_t pass = 0; pass <= R; ++pass) {
        bool changed = false;
        for (size_t r = 0; r < R; ++r) {
            int32_t lv = 0;
            bool ready = true;
            for (int32_t k = tb.up_off[r]; k < tb.up_off[r + 1]; ++k) {
                const int32_t ul = level[size_t(tb.ups[size_t(k)])];
                if (ul < 0) { ready = false; break; }
                lv = std::max(lv, ul + 1);
            }
            if (ready && level[r] != lv) { level[r] = lv; changed = true; }
        }
        if (!changed) break;
    }
    int32_t n_levels = 0;
    for (size_t r = 0; r < R; ++r) {
        if (level[r] < 0) return false;
        n_levels = std::max(n_levels, level[r] + 1);
    }
    build_csr(size_t(n_levels), tb.lvl_off, tb.lvl_rivers, [&](auto&& emit) {
        for (size_t r = 0; r < R; ++r) emit(size_t(level[r]), int32_t(r));
    });
    return true;
}

}  // namespace shyft_hip_impl
