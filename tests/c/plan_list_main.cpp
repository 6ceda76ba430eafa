// plan_list_main.cpp -- runs tv_plan.h's launch order of a v1 list (list_plan) on the CPU for tests/test_plan_list.py
// (g++; no HIP; may be built with -fsanitize=address,undefined).
// stdin, one query per line:
//   l n short_last heldf  piece_0 .. piece_n-1  [held_0 .. held_n-1]
//     short_last: the shard-relative index of the short last piece, -1 = none.  heldf = 1: n held flags (0 / 1) follow;
//     0: held is NULL (every entry holds a slot).
//   -> "m piece:origin .."        (launch[t]:origin[t] for the m launch positions)
#include <cinttypes>
#include <cstdio>

#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind != 'l') return 2;
        uint64_t n;
        int64_t last;
        int heldf;
        if (std::scanf("%" SCNu64 " %" SCNd64 " %d", &n, &last, &heldf) != 3) return 2;
        std::vector<uint32_t> pieces(n);
        for (auto& v : pieces)
            if (std::scanf("%" SCNu32, &v) != 1) return 2;
        std::vector<uint8_t> held;
        if (heldf)
            for (uint64_t k = 0; k < n; k++) {
                int v;
                if (std::scanf("%d", &v) != 1) return 2;
                held.push_back((uint8_t)v);
            }
        std::vector<uint32_t> launch{7, 7, 7};   // (the plan replaces what the vectors held)
        std::vector<int64_t> origin{1};
        tvi::list_plan(n, pieces.data(), heldf ? held.data() : nullptr, last < 0 ? UINT64_MAX : (uint64_t)last, &launch,
                       &origin);
        if (launch.size() != origin.size()) return 3;
        std::printf("%zu", launch.size());
        for (size_t t = 0; t < launch.size(); t++) std::printf(" %" PRIu32 ":%" PRId64, launch[t], origin[t]);
        std::printf("\n");
    }
    return 0;
}
