// plan_batch_main.cpp -- runs tv_plan.h's launch order and group geometry of a batch (batch_plan) on the CPU for
// tests/test_plan_batch.py (g++; no HIP; may be built with -fsanitize=address,undefined).
// stdin, one query per line:
//   b span n  len_0 .. len_n-1
//   -> "m g  entry:origin ..  fast_end:end:nb_min .."   (the m launch positions, then the g group records)
#include <cinttypes>
#include <cstdio>

#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind != 'b') return 2;
        uint32_t span;
        uint64_t n;
        if (std::scanf("%" SCNu32 " %" SCNu64, &span, &n) != 2) return 2;
        std::vector<uint64_t> lens(n);
        for (auto& v : lens)
            if (std::scanf("%" SCNu64, &v) != 1) return 2;
        std::vector<uint32_t> launch{7, 7, 7};   // (the plan replaces what the vectors held)
        std::vector<int64_t> origin{1};
        std::vector<tvi::BatchGroup> groups(2);
        tvi::batch_plan(n, lens.data(), span, &launch, &origin, &groups);
        if (launch.size() != origin.size()) return 3;
        std::printf("%zu %zu", launch.size(), groups.size());
        for (size_t t = 0; t < launch.size(); t++) std::printf(" %" PRIu32 ":%" PRId64, launch[t], origin[t]);
        for (const tvi::BatchGroup& q : groups) std::printf(" %" PRIu32 ":%" PRIu32 ":%" PRIu32, q.fast_end, q.end, q.nb_min);
        std::printf("\n");
    }
    return 0;
}
