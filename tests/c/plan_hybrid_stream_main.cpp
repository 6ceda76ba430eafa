// plan_hybrid_stream_main.cpp -- runs tv_plan.h's hybrid stream planning on the CPU for tests/test_plan_hybrid_stream.py
// (g++; no HIP; may be built with -fsanitize=address,undefined).
// stdin, one query per line:
//   g L count budget chunk                      -> "C wn"                    (hybrid_stream_geometry, slack 256)
//   r piece_bytes v1_len offset C               -> "b e chunks"              (hybrid_col_range, hybrid_col_chunks)
//   p total L first count offset C align  pb_0 .. pb_count-1
//     Replays the column pad launch of the unit rows [0, count) x column [offset, offset + C) on a host buffer: rows of
//     pitch C + 256 at base + j * pitch with base = align mod 16 past a 16-byte boundary, one guard row on either side,
//     every byte 0xFF before; workgroup (row, k), k below the most chunks a row has, does what
//     tv_hybrid_col_pad_kernel's does (hybrid_col_chunk, hybrid_split; byte stores, 16-byte stores, byte stores).  A store
//     outside the unit's rows, a 16-byte store at an unaligned address, or a byte stored twice ends the program with a
//     non-zero status.
//     -> "chunks | a:b .." : the grid's chunk count, then per row the half-open range of zero bytes in [0, pitch)
//        ("-" = none; "x" = the zero bytes are not one range); a guard row that changed prints "guard"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'g') {
            uint64_t L, count, budget, chunk, C = 0, wn = 0;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &L, &count, &budget, &chunk) != 4) return 2;
            tvi::hybrid_stream_geometry(L, count, budget, chunk, 256, &C, &wn);
            std::printf("%" PRIu64 " %" PRIu64 "\n", C, wn);
            continue;
        }
        if (kind == 'r') {
            uint64_t pb, v1, offset, C, b = 0, e = 0;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &pb, &v1, &offset, &C) != 4) return 2;
            tvi::hybrid_col_range(pb, v1, offset, C, &b, &e);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", b, e, tvi::hybrid_col_chunks(b, e));
            continue;
        }
        if (kind != 'p') return 2;
        uint64_t total, L, first, count, offset, C, align;
        if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &total, &L,
                       &first, &count, &offset, &C, &align) != 7)
            return 2;
        std::vector<uint32_t> pb(count);
        for (auto& v : pb)
            if (std::scanf("%" SCNu32, &v) != 1) return 2;
        if (align > 15 || C == 0) return 2;
        const uint64_t pitch = C + 256;
        std::vector<uint8_t> raw((count + 2) * pitch + 64, 0xFF);
        const uint64_t base = (reinterpret_cast<uint64_t>(raw.data()) + 31) / 16 * 16 + align;   // `align` mod 16
        const uint64_t lo = base + pitch, hi = lo + count * pitch;                               // the unit's rows
        auto store = [&](uint64_t a, uint64_t n) {
            if (a < lo || a + n > hi) std::exit(5);
            if (n == 16 && a % 16) std::exit(6);
            uint8_t* q = reinterpret_cast<uint8_t*>(a);
            for (uint64_t k = 0; k < n; k++) {
                if (q[k] != 0xFF) std::exit(7);
                q[k] = 0;
            }
        };
        uint64_t chunks = 0;   // as the host sizes the grid
        for (uint64_t r = 0; r < count; r++) {
            uint64_t b, e;
            tvi::hybrid_col_range(pb[r], tvi::hybrid_v1_len(total, L, first + r), offset, C, &b, &e);
            chunks = std::max(chunks, tvi::hybrid_col_chunks(b, e));
        }
        for (uint64_t r = 0; r < count; r++)
            for (uint64_t k = 0; k < chunks; k++) {
                uint64_t b, e;
                if (!tvi::hybrid_col_chunk(pb[r], total, L, first + r, offset, C, (uint32_t)k, &b, &e)) continue;
                const uint64_t row = lo + r * pitch, a = row + b, z = row + e;
                uint64_t va, ve;
                tvi::hybrid_split(a, z, &va, &ve);
                for (uint64_t tid = 0; tid < 256; tid++) {
                    if (a + tid < va) store(a + tid, 1);
                    for (uint64_t q = va + 16 * tid; q < ve; q += 16 * 256) store(q, 16);
                    if (ve + tid < z) store(ve + tid, 1);
                }
            }
        std::printf("%" PRIu64 " |", chunks);
        bool guard = false;
        for (uint64_t k = 0; k < pitch; k++)
            guard = guard || reinterpret_cast<const uint8_t*>(base)[k] != 0xFF ||
                    reinterpret_cast<const uint8_t*>(hi)[k] != 0xFF;
        if (guard) std::printf(" guard");
        for (uint64_t j = 0; j < count; j++) {
            const uint8_t* r = reinterpret_cast<const uint8_t*>(lo + j * pitch);
            uint64_t a = pitch, z = 0, zeros = 0;
            for (uint64_t k = 0; k < pitch; k++)
                if (r[k] == 0) {
                    if (a == pitch) a = k;
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
