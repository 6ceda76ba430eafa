// fileio_main.cpp -- runs tv_fileio.h's read primitives and tv_plan.h's path-table parser, slot packing and copy
// runs on the CPU for tests/test_fileio.py (g++; no HIP; may be built with -fsanitize=address,undefined).
// stdin, one query per line ("hex" is "-" for no bytes):
//   r path off need ask      -> read_at on the file (O_RDONLY):           "count hex" (hex: the count bytes) or "-errno"
//   x path off need ask      -> read_at on a descriptor closed before it: the same
//   q fo n                   -> direct_request:                           "al lead ask"
//   d path fo len step       -> read_direct (dst 4 KiB-aligned):          "count hex" or "-errno"
//   t n threads              -> pread_part:                               "part"
//   p n hex                  -> parse_path_table over exactly those bytes: "count off_0 .. off_count-1"
//   s slot m  lin_0 len_0 ok_0 .. lin_m-1 len_m-1 ok_m-1
//                            -> pack_slot from segment 0 on and for_copy_runs per slot, one token group per slot:
//                               "i j packed_i .. packed_j-1 / q:r q:r .. ;"
#include <fcntl.h>
#include <unistd.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include <string>
#include <vector>

#include "../../torrent_amd/csrc/tv_fileio.h"
#include "../../torrent_amd/csrc/tv_plan.h"

static void print_read(int64_t got, const uint8_t* p) {
    std::printf("%" PRId64 " ", got);
    for (int64_t i = 0; i < got; i++) std::printf("%02x", p[i]);
    std::printf(got > 0 ? "\n" : "-\n");
}

int main() {
    char kind;
    char path[4096];
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'r' || kind == 'x') {
            uint64_t off, need, ask;
            if (std::scanf("%4095s %" SCNu64 " %" SCNu64 " %" SCNu64, path, &off, &need, &ask) != 4 || ask < need) return 2;
            const int fd = open(path, O_RDONLY);
            if (fd < 0) return 3;
            if (kind == 'x') close(fd);
            std::vector<uint8_t> buf(ask);               // (exactly what the loop may write: a byte more is an error)
            print_read(tvi::read_at(fd, buf.data(), off, need, ask), buf.data());
            if (kind == 'r') close(fd);
        } else if (kind == 'q') {
            uint64_t fo, n;
            if (std::scanf("%" SCNu64 " %" SCNu64, &fo, &n) != 2) return 2;
            const tvi::DirectReq r = tvi::direct_request(fo, n);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", r.al, r.lead, r.ask);
        } else if (kind == 'd') {
            uint64_t fo, len, step;
            if (std::scanf("%4095s %" SCNu64 " %" SCNu64 " %" SCNu64, path, &fo, &len, &step) != 4) return 2;
            const int fd = open(path, O_RDONLY);
            if (fd < 0) return 3;
            void* dst = nullptr;
            if (posix_memalign(&dst, 4096, len ? len : 1)) return 3;
            print_read(tvi::read_direct(fd, fo, (uint8_t*)dst, len, step), (const uint8_t*)dst);
            free(dst);
            close(fd);
        } else if (kind == 't') {
            uint64_t n;
            int threads;
            if (std::scanf("%" SCNu64 " %d", &n, &threads) != 2) return 2;
            std::printf("%" PRIu64 "\n", tvi::pread_part(n, threads));
        } else if (kind == 'p') {
            uint64_t n;
            static char hex[1 << 16];
            if (std::scanf("%" SCNu64 " %65535s", &n, hex) != 2) return 2;
            const std::string h = hex[0] == '-' ? "" : hex;
            std::vector<char> blob(h.size() / 2);        // (on the heap, exactly paths_bytes long)
            for (size_t i = 0; i < blob.size(); i++) {
                unsigned v;
                if (std::sscanf(h.c_str() + 2 * i, "%2x", &v) != 1) return 2;
                blob[i] = (char)v;
            }
            std::vector<const char*> out(n ? n : 1, nullptr);
            const uint64_t k = tvi::parse_path_table(n, blob.data(), blob.size(), out.data());
            std::printf("%" PRIu64, k);
            for (uint64_t q = 0; q < k; q++) std::printf(" %td", out[q] - blob.data());
            std::printf("\n");
        } else if (kind == 's') {
            uint64_t slot, m;
            if (std::scanf("%" SCNu64 " %" SCNu64, &slot, &m) != 2) return 2;
            std::vector<tvi::SmallSeg> s(m);
            std::vector<int> ok(m);
            for (uint64_t q = 0; q < m; q++) {
                if (std::scanf("%" SCNu64 " %" SCNu64 " %d", &s[q].linear, &s[q].len, &ok[q]) != 3) return 2;
                s[q].k = q;
                s[q].file_offset = 0;
                s[q].packed = UINT64_MAX;
            }
            for (size_t i = 0; i < s.size();) {
                const size_t j = tvi::pack_slot(s, i, slot);
                if (j == i) return 3;                    // (a segment longer than a slot is the test's mistake)
                std::printf("%zu %zu", i, j);
                for (size_t q = i; q < j; q++) std::printf(" %" PRIu64, s[q].packed);
                std::printf(" /");
                const int rc = tvi::for_copy_runs(s, i, j, [&](size_t q) { return ok[q] != 0; }, [&](size_t q, size_t r) {
                    std::printf(" %zu:%zu", q, r);
                    return 0;
                });
                if (rc) return 4;
                std::printf(" ; ");
                i = j;
            }
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
