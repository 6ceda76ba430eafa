// plan_codec_main.cpp -- runs tv_plan.h's digest-word codec on the CPU for tests/test_plan_codec.py (g++; no HIP; may
// be built with -fsanitize=address,undefined).
// stdin, one query per line:
//   c words tabwords n  base_0 pitch_0 col_0 .. base_n-1 pitch_n-1 col_n-1  hex
//     hex: the n digests of 4 x words bytes each, one after the other ("-" when n = 0).  Digest t is packed into the
//     table of row length pitch_t that starts at word base_t of a table of tabwords words, column col_t.
//   -> "word_0 .. word_tabwords-1 | hex"     (the table after every pack, words in hex, a word no pack wrote reads
//                                             eeeeeeee; then every digest unpacked from its place, one after the other)
#include <cinttypes>
#include <cstdio>

#include <string>
#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind != 'c') return 2;
        uint32_t words;
        uint64_t tabwords, n;
        if (std::scanf("%" SCNu32 " %" SCNu64 " %" SCNu64, &words, &tabwords, &n) != 3) return 2;
        std::vector<uint64_t> at(3 * n);
        for (auto& v : at)
            if (std::scanf("%" SCNu64, &v) != 1) return 2;
        const uint64_t len = 4ull * words;
        std::string hex(2 * n * len + 2, '\0');
        if (std::scanf("%s", &hex[0]) != 1) return 2;
        std::vector<uint8_t> in(n * len);
        for (uint64_t i = 0; i < in.size(); i++) {
            unsigned v;
            if (std::sscanf(hex.c_str() + 2 * i, "%2x", &v) != 1) return 2;
            in[i] = (uint8_t)v;
        }
        for (uint64_t t = 0; t < n; t++)   // (a query that would write outside the table is the test's mistake)
            if (at[3 * t + 2] >= at[3 * t + 1] || at[3 * t] + (words - 1) * at[3 * t + 1] + at[3 * t + 2] >= tabwords) return 3;
        std::vector<uint32_t> tab(tabwords, 0xEEEEEEEEu);
        for (uint64_t t = 0; t < n; t++)
            tvi::digest_pack(in.data() + t * len, words, tab.data() + at[3 * t], at[3 * t + 1], at[3 * t + 2]);
        std::vector<uint8_t> out(n * len + 1, 0xEE);   // (the unpack must write every byte of a digest, and no more)
        for (uint64_t t = n; t-- > 0;) {               // last first: a write past a digest's end would hit the next one
            tvi::digest_unpack(tab.data() + at[3 * t], at[3 * t + 1], at[3 * t + 2], words, out.data() + t * len);
            if (out[(t + 1) * len] != (t + 1 < n ? in[(t + 1) * len] : 0xEE)) return 4;
        }
        for (uint32_t v : tab) std::printf("%08" PRIx32 " ", v);
        std::printf("| ");
        for (uint64_t i = 0; i < n * len; i++) std::printf("%02x", out[i]);
        std::printf("\n");
    }
    return 0;
}
