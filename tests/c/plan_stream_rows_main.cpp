// plan_stream_rows_main.cpp -- runs tv_plan.h's two pure rules of the stream engine on the CPU for
// tests/test_plan_stream_rows.py (g++; no HIP; may be built with -fsanitize=address,undefined): a request's copy plan
// (for_row_copies) and a row's walk over the file table (walk_row_files).
// stdin, one query per line:
//   c width src_pitch stop n  b_0 .. b_n-1
//     The copy plan of n rows of `width` bytes, row q holding b_q valid ones; the emit of index `stop` (-1: none)
//     returns 7.  Each emit is replayed on host buffers as stream_commit_locked queues it (a full run: `rows` rows of
//     `width` bytes from source pitch src_pitch to destination pitch width + 256; a short row: one copy of its bytes).
//     The source holds exactly the rows' valid bytes (row q at q * src_pitch) and nothing after the last of them; the
//     destination is n rows and one guard row on either side, every byte 0xFF before.
//     -> "ret | first:rows:bytes .. | ok" ("-" for no emit; "diff" when the destination is not the row-by-row copy of
//        each row's valid bytes with every other byte untouched; stop >= 0: the rows from the stopped emit on are not
//        expected)
//   w L a b stop n  len_0 .. len_n-1
//     The walk of LINEAR bytes [a, b) over n files of these lengths, back to back (L == 0) or each at the next multiple
//     of L (v2_file_starts); the seg call of index `stop` (-1: none) returns false.
//     -> "result | file:file_offset:dst_offset:len .." (result: 0 walked, 1 gap, 2 short; "-" for no segment)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

static int copy_plan() {
    uint64_t width, spitch, n;
    int64_t stop;
    if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNu64, &width, &spitch, &stop, &n) != 4) return 2;
    std::vector<uint64_t> b(n);
    for (auto& v : b)
        if (std::scanf("%" SCNu64, &v) != 1 || v > width) return 2;
    if (!spitch || (n > 1 && spitch < width)) return 2;
    uint64_t src_bytes = 0;
    for (uint64_t q = 0; q < n; q++)
        if (b[q]) src_bytes = q * spitch + b[q];
    std::vector<uint8_t> src(src_bytes);
    for (uint64_t k = 0; k < src_bytes; k++) src[k] = (uint8_t)((k * 131 + k / spitch * 7 + 1) % 251);   // never 0xFF
    const uint64_t dpitch = width + 256;
    std::vector<uint8_t> dst((n + 2) * dpitch, 0xFF), want(dst);
    uint8_t* d0 = dst.data() + dpitch;
    int64_t emits = 0;
    uint64_t covered = n;   // rows [0, covered) are expected in the destination
    std::vector<uint64_t> out;
    const int ret = tvi::for_row_copies(n, width, [&](uint64_t q) { return b[q]; },
                                        [&](uint64_t q, uint64_t rows, uint64_t nb) -> int {
        out.insert(out.end(), {q, rows, nb});
        if (emits++ == stop) {
            covered = q;
            return 7;
        }
        if (nb == width)
            for (uint64_t r = 0; r < rows; r++) memcpy(d0 + (q + r) * dpitch, src.data() + (q + r) * spitch, width);
        else
            memcpy(d0 + q * dpitch, src.data() + q * spitch, nb);
        return 0;
    });
    for (uint64_t q = 0; q < covered; q++)
        if (b[q]) memcpy(want.data() + (q + 1) * dpitch, src.data() + q * spitch, b[q]);
    std::printf("%d |", ret);
    for (size_t k = 0; k < out.size(); k += 3) std::printf(" %" PRIu64 ":%" PRIu64 ":%" PRIu64, out[k], out[k + 1], out[k + 2]);
    if (out.empty()) std::printf(" -");
    std::printf(" | %s\n", dst == want ? "ok" : "diff");
    return 0;
}

static int row_walk() {
    uint64_t L, a, b, n;
    int64_t stop;
    if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNu64, &L, &a, &b, &stop, &n) != 5) return 2;
    std::vector<uint64_t> len(n), start(n + 1, 0);
    for (auto& v : len)
        if (std::scanf("%" SCNu64, &v) != 1) return 2;
    uint64_t bad = 0;
    if (L) {
        if (!tvi::v2_file_starts(n, len.data(), L, &start, &bad)) return 2;
    } else {
        for (uint64_t k = 0; k < n; k++) start[k + 1] = start[k] + len[k];
    }
    int64_t segs = 0;
    std::vector<uint64_t> out;
    const tvi::RowWalk w = tvi::walk_row_files(start.data(), len.data(), n, a, b,
                                               [&](uint64_t k, uint64_t fo, uint64_t at, uint64_t l) {
        out.insert(out.end(), {k, fo, at, l});
        return segs++ != stop;
    });
    std::printf("%d |", (int)w);
    for (size_t k = 0; k < out.size(); k += 4)
        std::printf(" %" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64, out[k], out[k + 1], out[k + 2], out[k + 3]);
    if (out.empty()) std::printf(" -");
    std::printf("\n");
    return 0;
}

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        const int rc = kind == 'c' ? copy_plan() : kind == 'w' ? row_walk() : 2;
        if (rc) return rc;
    }
    return 0;
}
