// plan_stream_main.cpp -- runs tv_plan.h's v1 stream planning on the CPU for tests/test_v1_columns_shapes.py (g++; no HIP).
// stdin, one query per line:
//   L count budget min_win   -> "C win"   (stream_geometry; one 64 MiB ring slot and slack 256, as the library passes them)
#include <cinttypes>
#include <cstdio>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    uint64_t L, count, budget, min_win;
    while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &L, &count, &budget, &min_win) == 4) {
        uint64_t C = 0, win = 0;
        tvi::stream_geometry(L, count, budget, min_win, 64ull << 20, 256, &C, &win);
        std::printf("%" PRIu64 " %" PRIu64 "\n", C, win);
    }
    return 0;
}
