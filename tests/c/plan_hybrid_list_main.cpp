// plan_hybrid_list_main.cpp -- replays the pad launch of a hybrid list call (tv_hybrid_verify_list) on the CPU for
// tests/test_plan_hybrid_list.py (g++; no HIP; may be built with -fsanitize=address,undefined).
// stdin, one query per line:
//   c piece_bytes total L piece                 -> "chunks"                  (hybrid_list_chunks)
//   p total L stride nrows n  row_0 piece_0 pb_0 .. row_n-1 piece_n-1 pb_n-1
//     A payload of nrows rows (slots) of `stride` bytes, its base 64-byte aligned as the library's is, one guard row on
//     either side, every byte 0xFF before.  Entry k lists GLOBAL piece piece_k with pb_k file bytes, held in row row_k.
//     Workgroup (entry, chunk), chunk below the most chunks an entry has (as the host sizes the grid), does what
//     tv_hybrid_list_pad_kernel's does (hybrid_list_chunk, hybrid_split; byte stores, 16-byte stores, byte stores; an
//     entry whose row is outside the payload is skipped).  A store outside the payload's rows or a 16-byte store at an
//     unaligned address ends the program with a non-zero status.
//     -> "chunks | a:z:lo:hi .." : the grid's chunk count, then per ROW the half-open range of zero bytes in
//        [0, stride) and the fewest and the most stores any byte of it got ("-" = no zero byte; "x" = the zero bytes are
//        not one range); a guard row that changed prints "guard"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'c') {
            uint64_t pb, total, L, piece;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &pb, &total, &L, &piece) != 4) return 2;
            std::printf("%" PRIu64 "\n", tvi::hybrid_list_chunks(pb, total, L, piece));
            continue;
        }
        if (kind != 'p') return 2;
        uint64_t total, L, stride, nrows, n;
        if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &total, &L, &stride, &nrows, &n) != 5)
            return 2;
        std::vector<uint32_t> row(n), pb(n);
        std::vector<uint64_t> piece(n);
        for (uint64_t k = 0; k < n; k++)
            if (std::scanf("%" SCNu32 " %" SCNu64 " %" SCNu32, &row[k], &piece[k], &pb[k]) != 3) return 2;
        if (stride < L || stride % 64 || nrows == 0) return 2;
        std::vector<uint8_t> raw((nrows + 2) * stride + 128, 0xFF);
        std::vector<uint8_t> count(raw.size(), 0);
        const uint64_t base = (reinterpret_cast<uint64_t>(raw.data()) + 63) / 64 * 64;
        const uint64_t lo = base + stride, hi = lo + nrows * stride;   // the payload's rows
        auto store = [&](uint64_t a, uint64_t len) {
            if (a < lo || a + len > hi) std::exit(5);
            if (len == 16 && a % 16) std::exit(6);
            uint8_t* q = reinterpret_cast<uint8_t*>(a);
            for (uint64_t k = 0; k < len; k++) {
                q[k] = 0;
                count[a + k - reinterpret_cast<uint64_t>(raw.data())]++;
            }
        };
        uint64_t chunks = 0;   // as the host sizes the grid
        for (uint64_t k = 0; k < n; k++) chunks = std::max(chunks, tvi::hybrid_list_chunks(pb[k], total, L, piece[k]));
        for (uint64_t en = 0; en < n; en++)
            for (uint64_t k = 0; k < chunks; k++) {
                uint64_t b, e;
                if (row[en] >= nrows || !tvi::hybrid_list_chunk(pb[en], total, L, piece[en], (uint32_t)k, &b, &e)) continue;
                const uint64_t r = lo + row[en] * stride, a = r + b, z = r + e;
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
        for (uint64_t k = 0; k < stride; k++)
            guard = guard || reinterpret_cast<const uint8_t*>(base)[k] != 0xFF ||
                    reinterpret_cast<const uint8_t*>(hi)[k] != 0xFF;
        if (guard) std::printf(" guard");
        for (uint64_t j = 0; j < nrows; j++) {
            const uint8_t* r = reinterpret_cast<const uint8_t*>(lo + j * stride);
            const uint8_t* cnt = count.data() + (lo + j * stride - reinterpret_cast<uint64_t>(raw.data()));
            uint64_t a = stride, z = 0, zeros = 0;
            unsigned cmin = 255, cmax = 0;
            for (uint64_t k = 0; k < stride; k++)
                if (r[k] == 0) {
                    if (a == stride) a = k;
                    z = k + 1;
                    zeros++;
                    cmin = std::min<unsigned>(cmin, cnt[k]);
                    cmax = std::max<unsigned>(cmax, cnt[k]);
                }
            if (!zeros) std::printf(" -");
            else if (zeros != z - a) std::printf(" x");
            else std::printf(" %" PRIu64 ":%" PRIu64 ":%u:%u", a, z, cmin, cmax);
        }
        std::printf("\n");
    }
    return 0;
}
