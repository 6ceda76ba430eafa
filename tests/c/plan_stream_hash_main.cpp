// plan_stream_hash_main.cpp -- prints what tv_plan.h says about a v2 stream's device table (v2s_tab_words,
// v2s_hash_words, v2s_hash_base, v2s_hash_word, v2s_nodes_b_base) for tests/test_plan_stream_hash.py.  An ordinary
// executable with no GPU code: it also builds with -fsanitize=address,undefined.
//
// stdin, one query per line:  r <count> <wn> <ncol>
// stdout, one line per query: the table's words, the hash region's words, then for every window its base in the table
// and the word at which level buffer B of its top tree starts ("w <base> <b_base>"), then for every shard piece j and
// q = 0 .. 7 the word of the hash region that holds hash word q of piece j ("i" and 8 x count numbers, piece-major).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

int main() {
    char op;
    unsigned long long count, wn, ncol;
    while (scanf(" %c %llu %llu %llu", &op, &count, &wn, &ncol) == 4) {
        if (op != 'r' || !count || !wn || !ncol) return 2;
        printf("%llu %llu", (unsigned long long)tvi::v2s_tab_words(count), (unsigned long long)tvi::v2s_hash_words(count));
        for (uint64_t j0 = 0; j0 < count; j0 += wn) {
            const uint64_t wcount = wn < count - j0 ? wn : count - j0;
            printf(" w %llu %llu", (unsigned long long)tvi::v2s_hash_base(count, j0),
                   (unsigned long long)tvi::v2s_nodes_b_base(wcount, ncol));
        }
        printf(" i");
        // (a host vector of exactly the region's size: an index outside it is caught by the sanitizer build)
        std::vector<uint8_t> seen(tvi::v2s_hash_words(count), 0);
        for (uint64_t j = 0; j < count; j++)
            for (uint32_t q = 0; q < 8; q++) {
                const uint64_t w = tvi::v2s_hash_word(count, wn, j, q);
                seen.at(w)++;
                printf(" %llu", (unsigned long long)w);
            }
        printf("\n");
    }
    return 0;
}
