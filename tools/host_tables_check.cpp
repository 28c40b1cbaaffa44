// Check of shyft_amd/csrc/include_internal/host_tables.h (the CSR builder and the river network tables) on the CPU,
// under the address and undefined-behaviour sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o host_tables_check tools/host_tables_check.cpp && ./host_tables_check
//
// build_csr on a hand-made case with an empty key and a skipped item, on an identity and a non-identity input, with
// both offset types, with no keys, and with an enumeration that throws; build_river_tables on the 2-cycle, the 3-cycle
// and the 7-river network of tests/test_routing_edges.py, for one member and for two. It prints the number of checks
// and returns non-zero at the first that fails; the sanitizers abort on any finding. Host code only
// (tests/test_host_tables.py builds and runs it).
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "../shyft_amd/csrc/include_internal/host_tables.h"

using namespace shyft_hip_impl;

namespace {

int n_checks = 0;

template <class T>
void expect(const char* what, const std::vector<T>& got, std::vector<long long> want) {
    ++n_checks;
    bool ok = got.size() == want.size();
    for (size_t i = 0; ok && i < want.size(); ++i) ok = (long long)got[i] == want[i];
    if (ok) return;
    std::printf("FAILED %s: got", what);
    for (const T& v : got) std::printf(" %lld", (long long)v);
    std::printf("\n");
    std::exit(1);
}
void expect(const char* what, bool got, bool want) { expect(what, std::vector<int>{got}, {want}); }

template <class Off>
void csr_cases() {
    std::vector<Off> off;
    std::vector<int32_t> items;
    // keys of items 0..6; item 3 is skipped, key 1 stays empty; within a key the items keep their order
    const int key_of[7] = {2, 0, 2, -1, 3, 0, 2};
    bool id = build_csr(4, off, items, [&](auto&& emit) {
        for (int i = 0; i < 7; ++i)
            if (key_of[i] >= 0) emit(size_t(key_of[i]), int32_t(i));
    });
    expect("csr off", off, {0, 2, 2, 5, 6});
    expect("csr items", items, {1, 5, 0, 2, 6, 4});
    expect("csr identity", id, false);
    // contiguous keys in item order: the identity
    id = build_csr(3, off, items, [&](auto&& emit) {
        for (int i = 0; i < 6; ++i) emit(size_t(i / 2), int32_t(i));
    });
    expect("identity off", off, {0, 2, 4, 6});
    expect("identity items", items, {0, 1, 2, 3, 4, 5});
    expect("identity", id, true);
    // a skipped last item leaves a shorter identity: the caller compares the length
    id = build_csr(2, off, items, [&](auto&& emit) {
        emit(0, 0);
        emit(1, 1);
    });
    expect("short identity", id, true);
    expect("short identity items", items, {0, 1});
    // item i % 3: not the identity although every key has its items
    id = build_csr(3, off, items, [&](auto&& emit) {
        for (int i = 0; i < 6; ++i) emit(size_t(i % 3), int32_t(i));
    });
    expect("permuted items", items, {0, 3, 1, 4, 2, 5});
    expect("permuted identity", id, false);
    id = build_csr(0, off, items, [&](auto&&) {});
    expect("no keys off", off, {0});
    expect("no keys items", items, {});
    expect("no keys identity", id, true);
    bool thrown = false;
    try {
        build_csr(2, off, items, [&](auto&& emit) {
            emit(1, 0);
            throw std::runtime_error("refused");
        });
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    expect("enumeration throws", thrown, true);
}

template <class Off>
void network_cases() {
    river_tables<Off> tb;
    const int64_t one[2] = {0, 1};
    const int32_t on_river_0[1] = {0};
    const int32_t cycle2[3] = {1, 0, -1}, cycle3[4] = {1, 2, 0, 0};
    expect("2-cycle", build_river_tables(1, one, on_river_0, 3, cycle2, tb), false);
    expect("3-cycle", build_river_tables(1, one, on_river_0, 4, cycle3, tb), false);
    // 7 rivers on 4 levels: 0, 4, 6 -> 1 -> 5 -> 3, river 2 on its own
    const int32_t down[7] = {1, 5, -1, -1, 1, 3, 1};
    const int32_t group_river[12] = {0, 6, 1, 4, 0, 3, 2, 1, 3, 2, 1, 4};
    const int64_t all[2] = {0, 12};
    expect("tree", build_river_tables(1, all, group_river, 7, down, tb), true);
    expect("tree pair_off", tb.pair_off, {0, 2, 5, 7, 9, 11, 11, 12});
    expect("tree pair_groups", tb.pair_groups, {0, 4, 2, 7, 10, 6, 9, 5, 8, 3, 11, 1});
    expect("tree up_off", tb.up_off, {0, 0, 3, 3, 4, 4, 5, 5});
    expect("tree ups", tb.ups, {0, 4, 6, 5, 1});
    expect("tree lvl_off", tb.lvl_off, {0, 4, 5, 6, 7});
    expect("tree lvl_rivers", tb.lvl_rivers, {0, 2, 4, 6, 1, 5, 3});
    expect("tree levels", std::vector<int>{tb.n_levels()}, {4});
    // two members: rows [0, 5) and [5, 12); a (member, river) pair holds its member's rows only, ascending
    const int64_t two[3] = {0, 5, 12};
    expect("two members", build_river_tables(2, two, group_river, 7, down, tb), true);
    expect("two members pair_off", tb.pair_off, {0, 2, 3, 3, 3, 4, 4, 5, 5, 7, 9, 11, 12, 12, 12});
    expect("two members pair_groups", tb.pair_groups, {0, 4, 2, 3, 1, 7, 10, 6, 9, 5, 8, 11});
    expect("two members lvl_rivers", tb.lvl_rivers, {0, 2, 4, 6, 1, 5, 3});
    // a downstream below -1 is an outlet like -1 (shyft_hip_route takes it; route_members refuses it beforehand)
    const int32_t below[2] = {-5, 0};
    expect("downstream -5", build_river_tables(1, one, on_river_0, 2, below, tb), true);
    expect("downstream -5 ups", tb.ups, {1});
    expect("downstream -5 lvl_rivers", tb.lvl_rivers, {1, 0});
}

}  // namespace

int main() {
    csr_cases<int32_t>();
    csr_cases<int64_t>();
    network_cases<int32_t>();
    network_cases<int64_t>();
    std::printf("host_tables_check: %d checks passed\n", n_checks);
    return 0;
}
