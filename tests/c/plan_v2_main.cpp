// plan_v2_main.cpp -- runs tv_plan.h's v2 stream planning on the CPU for tests/test_plan_v2.py (g++; no HIP).
// stdin, one query per line:
//   g L count budget chunk   -> "C wn"            (v2_stream_geometry; slack 256, as the library passes it)
//   s L n len_0 .. len_n-1   -> "start_0 .. start_n" or "overflow k"   (v2_file_starts)
#include <cinttypes>
#include <cstdio>

#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'g') {
            uint64_t L, count, budget, chunk, C = 0, wn = 0;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &L, &count, &budget, &chunk) != 4) return 2;
            tvi::v2_stream_geometry(L, count, budget, chunk, 256, &C, &wn);
            std::printf("%" PRIu64 " %" PRIu64 "\n", C, wn);
        } else if (kind == 's') {
            uint64_t L, n;
            if (std::scanf("%" SCNu64 " %" SCNu64, &L, &n) != 2) return 2;
            std::vector<uint64_t> len(n), start;
            for (auto& v : len)
                if (std::scanf("%" SCNu64, &v) != 1) return 2;
            uint64_t bad = 0;
            if (!tvi::v2_file_starts(n, len.data(), L, &start, &bad)) {
                std::printf("overflow %" PRIu64 "\n", bad);
                continue;
            }
            for (size_t k = 0; k < start.size(); k++) std::printf("%s%" PRIu64, k ? " " : "", start[k]);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
