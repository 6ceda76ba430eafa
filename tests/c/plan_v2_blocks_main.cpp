// plan_v2_blocks_main.cpp -- runs tv_plan.h's v2 block item planning on the CPU for tests/test_plan_v2_blocks.py
// (g++; no HIP; may be built with -fsanitize=address,undefined).
// stdin, one query per line:
//   b W cap n want skipf  pb_0 .. pb_n-1  [row_0 .. row_n-1]  [skip_0 .. skip_n-1]  nb word_0 .. word_nb-1
//     want = 0: want_bits NULL; 1: n hex rows of ceil(W / 8) bytes follow.  skipf = 1: n skip flags (0 / 1) follow.
//     word_k: the launch's ballot word k in hex (bit l = item 64 k + l matched); nb must cover the items.
//   -> "over"                                           (more than cap items)
//   -> "m e:leaf:len .. | okrow_0 .. okrow_n-1"         (v2_block_items, then v2_block_scatter; rows in hex)
#include <cinttypes>
#include <cstdio>

#include <string>
#include <vector>

#include "../../torrent_amd/csrc/tv_plan.h"

static bool read_hex(std::vector<uint8_t>* out, size_t nbytes) {
    char buf[1 << 16];
    if (std::scanf("%65535s", buf) != 1) return false;
    const std::string s(buf);
    if (s.size() != 2 * nbytes) return false;
    for (size_t i = 0; i < nbytes; i++) {
        unsigned v;
        if (std::sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out->push_back((uint8_t)v);
    }
    return true;
}

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind != 'b') return 2;
        uint64_t W, cap, n, nb;
        int want, skipf;
        if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %d %d", &W, &cap, &n, &want, &skipf) != 5) return 2;
        const uint64_t pitch = tvi::v2_block_pitch(W);
        std::vector<uint32_t> pb(n);
        for (auto& v : pb)
            if (std::scanf("%" SCNu32, &v) != 1) return 2;
        std::vector<uint8_t> rows, skip;
        if (want)
            for (uint64_t k = 0; k < n; k++)
                if (!read_hex(&rows, pitch)) return 2;
        if (skipf)
            for (uint64_t k = 0; k < n; k++) {
                int v;
                if (std::scanf("%d", &v) != 1) return 2;
                skip.push_back((uint8_t)v);
            }
        if (std::scanf("%" SCNu64, &nb) != 1) return 2;
        std::vector<uint64_t> ballots(nb);
        for (auto& v : ballots)
            if (std::scanf("%" SCNx64, &v) != 1) return 2;
        std::vector<tvi::V2BlockItem> items;
        if (!tvi::v2_block_items(n, pb.data(), W, want ? rows.data() : nullptr, skipf ? skip.data() : nullptr, cap,
                                 &items)) {
            std::printf("over\n");
            continue;
        }
        if ((items.size() + 63) / 64 > nb) return 3;
        std::vector<uint8_t> ok(n * pitch + 1, 0xEE);   // (the scatter must write every byte of its rows, and no more)
        tvi::v2_block_scatter(n, W, items, ballots.data(), ok.data());
        if (ok[n * pitch] != 0xEE) return 4;
        std::printf("%zu", items.size());
        for (const auto& it : items) std::printf(" %" PRIu32 ":%" PRIu32 ":%" PRIu32, it.entry, it.leaf, it.len);
        std::printf(" |");
        for (uint64_t k = 0; k < n; k++) {
            std::printf(" ");
            for (uint64_t q = 0; q < pitch; q++) std::printf("%02x", ok[k * pitch + q]);
        }
        std::printf("\n");
    }
    return 0;
}
