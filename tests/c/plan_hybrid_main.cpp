// plan_hybrid_main.cpp -- runs tv_plan.h's hybrid tail planning on the CPU for tests/test_plan_hybrid.py (g++; no HIP;
// may be built with -fsanitize=address,undefined).
// stdin, one query per line:
//   t total L first count  pb_0 .. pb_count-1
//     -> "bad j"                                   (hybrid_tails refused: j = the shard piece, or "bad L")
//     -> "n chunks row:begin:end:chunk0 .."        (the tail table)
//   p total L first count stride align  pb_0 .. pb_count-1
//     Replays the pad launch on a host buffer: rows at base + j * stride with base = align mod 16 past a 16-byte
//     boundary, every byte 0xFF before; workgroup g = 0 .. chunks - 1 does what tv_hybrid_pad_kernel's does
//     (hybrid_chunk_entry, hybrid_chunk_range, hybrid_split; byte stores, 16-byte stores, byte stores).  A store
//     outside the buffer's rows, a 16-byte store at an unaligned address, or a byte stored twice ends the program
//     with a non-zero status.
//     -> "bad j" or "n chunks | a:b .." : per row the half-open range of zero bytes in [0, stride) ("-" = none;
//        "x" = the zero bytes are not one range)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind != 't' && kind != 'p') return 2;
        uint64_t total, L, first, count, stride = 0, align = 0;
        if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &total, &L, &first, &count) != 4) return 2;
        if (kind == 'p' && std::scanf("%" SCNu64 " %" SCNu64, &stride, &align) != 2) return 2;
        std::vector<uint32_t> pb(count);
        for (auto& v : pb)
            if (std::scanf("%" SCNu32, &v) != 1) return 2;
        std::vector<tvi::HybridTail> tails;
        uint64_t chunks = 0, bad = 0;
        if (!tvi::hybrid_tails(total, L, first, count, pb.data(), &tails, &chunks, &bad)) {
            if (bad == UINT64_MAX) std::printf("bad L\n");
            else std::printf("bad %" PRIu64 "\n", bad);
            continue;
        }
        std::printf("%zu %" PRIu64, tails.size(), chunks);
        if (kind == 't') {
            for (const auto& t : tails)
                std::printf(" %" PRIu32 ":%" PRIu32 ":%" PRIu32 ":%" PRIu32, t.row, t.begin, t.end, t.chunk0);
            std::printf("\n");
            continue;
        }
        if (stride < L || align > 15) return 2;
        // the rows, with 16 guard bytes on either side that no store may touch
        std::vector<uint8_t> raw(count * stride + 64, 0xFF);
        const uint64_t lo = (reinterpret_cast<uint64_t>(raw.data()) + 31) / 16 * 16 + align;   // base: `align` mod 16
        const uint64_t hi = lo + count * stride;
        auto store = [&](uint64_t a, uint64_t n) {
            if (a < lo || a + n > hi) std::exit(5);
            if (n == 16 && a % 16) std::exit(6);
            uint8_t* q = reinterpret_cast<uint8_t*>(a);
            for (uint64_t k = 0; k < n; k++) {
                if (q[k] != 0xFF) std::exit(7);
                q[k] = 0;
            }
        };
        for (uint64_t g = 0; g < chunks && !tails.empty(); g++) {
            const tvi::HybridTail t = tails[tvi::hybrid_chunk_entry(tails.data(), (uint32_t)tails.size(), (uint32_t)g)];
            uint64_t b, e;
            if (t.row >= count || t.end > L || !tvi::hybrid_chunk_range(t, (uint32_t)g, &b, &e)) continue;
            const uint64_t row = lo + (uint64_t)t.row * stride, a = row + b, z = row + e;
            uint64_t va, ve;
            tvi::hybrid_split(a, z, &va, &ve);
            for (uint64_t tid = 0; tid < 256; tid++) {
                if (a + tid < va) store(a + tid, 1);
                for (uint64_t q = va + 16 * tid; q < ve; q += 16 * 256) store(q, 16);
                if (ve + tid < z) store(ve + tid, 1);
            }
        }
        std::printf(" |");
        for (uint64_t j = 0; j < count; j++) {
            const uint8_t* r = reinterpret_cast<const uint8_t*>(lo + j * stride);
            uint64_t a = stride, z = 0, zeros = 0;
            for (uint64_t k = 0; k < stride; k++)
                if (r[k] == 0) {
                    if (a == stride) a = k;
                    z = k + 1;
                    zeros++;
                }
            if (!zeros) std::printf(" -");
            else if (zeros != z - a) std::printf(" x");
            else std::printf(" %" PRIu64 ":%" PRIu64, a, z);
        }
        std::printf("\n");
    }
    return 0;
}
