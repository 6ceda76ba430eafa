// tv_internal.h -- shared between the kernels (tv_kernels.hip) and the C ABI (tv_core.hip, tv_context.hip, ...: see tv_ctx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TV_KERNEL_AUTO 0
#define TV_KERNEL_LANE 1
#define TV_KERNEL_SPLIT 2
// (3 was MIX, a work queue over split pairs and lane waves: measured 8.6 % slower than lane where lane is
//  chosen, removed in round 3; the value stays unused)
#define TV_KERNEL_TWIN 4    // split with two lanes per piece in the rounds waves (half the K+W reads per block)

#ifndef TV_STAMPS
#define TV_STAMPS 0   // 1: diagnostic split-kernel loop stamps (tools/split_stamps.py), never the shipped library
#endif
// words of the device clock buffer (TV_OPT_CLOCK_PROBE): the probe's 4, plus in TV_STAMPS builds 8 per wave of up
// to 4 waves in each of 65,536 workgroups
constexpr size_t kClockWords = 4 + (TV_STAMPS ? 8 * 4 * 65536 : 0);

// The block ranges of one group of a batch launch (tv_plan.h batch_plan computes them; WaveGeom of tv_kernels.hip with
// fast_begin = 0): blocks [0, fast_end) are raw data for EVERY entry of the group (fast_end * 64 <= every length),
// blocks [.., end) are processed (the longest entry's count), every entry has at least nb_min blocks.
struct TvBatchGeom {
    uint32_t fast_end, end, nb_min, reserved;
};

// One launch over a contiguous run of n pieces.  Piece j's byte k (piece-relative) is at
// data + j*stride + k - data_off.  Blocks [blk_begin, min(blk_end, nb_j)) are processed.
struct TvPieces {
    const uint8_t* data;
    uint64_t stride;
    uint64_t data_off;
    uint64_t L;              // piece length of every piece except last_idx
    uint64_t last_len;       // length of piece last_idx
    uint64_t blk_begin;
    uint64_t blk_end;        // UINT64_MAX = through the end of every piece
    uint32_t n;
    uint32_t n_main;         // main groups cover pieces [0, n_main); n_main = n - 1 when the short last
                             // piece (last_len < L) gets a group of its own, else n (list mode: n)
    uint32_t last_idx;       // launch-local index of the torrent's last piece, 0xFFFFFFFF if absent
    uint32_t finalize;       // 1: compare / emit digests; 0: store chaining values to `state`
    uint32_t dcount;         // row stride of state / digests / out_digests (= shard piece count)
    uint32_t* state;         // [5][dcount] chaining values (read when blk_begin > 0, written when !finalize)
    const uint32_t* digests; // [5][dcount] expected digest words (big-endian values)
    const uint64_t* avail64; // MSB-first bitfield bytes over the shard (64-bit words); may be null
    uint64_t* out64;         // per 64 pieces, MSB-first bitfield bytes (sized to whole 256-piece groups)
    uint32_t* out_digests;   // hash mode: [5][dcount]
    const uint32_t* idx;     // list mode: lane j verifies shard piece idx[j] (data = base + idx*stride)
    uint8_t* out_bytes;      // list mode: out_bytes[j] = 1 iff piece idx[j] matches
    uint32_t fill_to;        // twin: launch this many workgroups in all (0 = the real grid only); the ones past
                             // the real grid are COMPANIONS that re-hash a main workgroup's pieces and discard
                             // the result (TV_OPT_TWIN_FILL)
    uint32_t fill_all;       // companions: 0 = every lane hashes the main workgroup's FIRST piece (the same
                             // instruction stream, 1/32 of the reads), 1 = its 32 pieces (TV_OPT_TWIN_FILL_READS)
    const uint32_t* rows;    // list mode with a slot pool (TV_OPT_LIST_SLOTS): entry j's bytes are payload row
                             // rows[j] (data + rows[j]*stride) while digests / length / availability stay those of
                             // piece idx[j]; null = row idx[j]
    uint64_t* clock;         // TV_OPT_CLOCK_PROBE: lane 0 of workgroup 0's (rounds) wave stores {shader clock counter,
                             // 100 MHz real-time counter} at its start and end here (4 words); null = off
    uint32_t lane_pairs;     // host-side choice for the lane kernel: 1 = the pair-load instantiation (a lane's two
                             // 64-B blocks of a 128-B line loaded back to back; >= 1 wave per SIMD), 0 = 3-deep ring
    // batch mode (tv_batch_verify: tv_launch_verify_batch): launch position j is a whole piece of ANY length, anywhere
    // in the payload; the positions are cut into groups of the kernel form's span by tv_plan.h batch_plan
    const uint64_t* b_off;   // [n] byte offset of position j's piece (its byte 0) from `data`
    const uint64_t* b_len;   // [n] its length
    const uint32_t* b_col;   // [n] its column in digests ([5][dcount])
    const TvBatchGeom* b_geom;   // [groups] the block ranges every wave of group g runs (uniform: loop bounds come from here only)
};

// ---- BitTorrent v2 (BEP 52): SHA-256 merkle piece roots over 16 KiB leaves (tv_v2_kernels.hip, tv_v2.hip) ----------
#define TV_KERNEL_V2 8      // tv_last_kernel id of tv_v2_verify / tv_v2_hash (leaf kernel + tree levels + finish)
#define TV_V2_MAP_LEAF 1    // lanes of a wave = consecutive leaves of one piece (16 KiB apart)
#define TV_V2_MAP_PIECE 2   // lanes of a wave = one leaf index of 64 consecutive pieces (`stride` apart)

// One v2 launch set over the n resident pieces of a shard.  Piece j's leaf k is the bytes at data + j*stride +
// k*16384; its hash goes to node slot j*W + k of level buffer A.  The tree levels ping-pong between A (row pitch W
// nodes per piece) and B (row pitch max(W/2, 1)); both are SoA [8][rows] words (big-endian values).
struct TvV2 {
    const uint8_t* data;
    uint64_t stride;
    uint32_t n;                  // pieces
    uint32_t logW;               // W = L / 16 KiB = 1 << logW leaves in a full piece
    uint32_t map;                // TV_V2_MAP_*
    const uint32_t* piece_bytes; // [n] valid bytes of piece j (1 .. L)
    const uint32_t* tree_leaves; // [n] width of piece j's tree (a power of two, >= its leaves, <= W)
    uint32_t* nodes_a;           // [8][n << logW]
    uint32_t* nodes_b;           // [8][n * max(W/2, 1)]
    const uint32_t* expect;      // verify: [8][n] expected root words
    uint32_t* roots;             // hash: [8][n] root words out
    const uint64_t* avail64;     // verify: MSB-first availability bytes in 64-bit words; may be null
    uint64_t* out64;             // verify: MSB-first bitfield bytes in 64-bit words, whole 256-piece groups
    uint64_t* clock;             // TV_OPT_CLOCK_PROBE (as TvPieces::clock); null = off
    uint32_t out_words;          // verify: the finish launch writes out64[0 .. out_words) only (a window of a streamed
                                 // shard: the words after it belong to the next window); 0 = every word of its grid
};
// Leaf hashes (every leaf inside a piece's valid bytes is hashed, the other positions of its tree get zero hashes).
hipError_t tv_v2_launch_leaves(const TvV2& p, hipStream_t s, uint32_t* workgroups);
// Tree level `level` (0 = leaves -> their parents) for every piece whose tree is wider than 1 << level; `maxlog` = the
// widest tree of the launch (log2).
hipError_t tv_v2_launch_level(const TvV2& p, uint32_t level, uint32_t maxlog, hipStream_t s);
// Roots: compare with `expect` and the availability into out64 (hash = false), or copy them to `roots`.
hipError_t tv_v2_launch_finish(const TvV2& p, bool hash, hipStream_t s);

// ---- the v2 list launch (tv_v2_verify_list): m self-describing entries, one kernel, no node buffers ---------------
#define TV_KERNEL_V2_LIST 16      // tv_last_kernel id of tv_v2_verify_list (tv_v2_list_kernel, one launch)
#define TV_V2_LIST_MAX_LOGW 16    // W up to 65,536 leaves (1 GiB pieces): the tile roots of one piece fill one LDS row
// Entry e's bytes are payload row rows[e] (data + rows[e] * stride): bytes[e] valid bytes, a tree of widths[e] leaves,
// the expected root in expect[q * m + e] (q = 0 .. 7, big-endian values).  out_bytes[e] = 1 iff the root matches.
struct TvV2List {
    const uint8_t* data;
    uint64_t stride;
    uint32_t m;                  // entries
    uint32_t logW;               // W = L / 16 KiB = 1 << logW: the widest tree an entry may have
    const uint32_t* rows;        // [m]
    const uint32_t* bytes;       // [m] 1 .. L
    const uint32_t* widths;      // [m] a power of two, ceil(bytes / 16 KiB) .. W
    const uint32_t* expect;      // [8][m]
    uint8_t* out_bytes;          // [m]
};
hipError_t tv_v2_launch_list(const TvV2List& p, hipStream_t s, uint32_t* workgroups);

// ---- the v2 column launch of a streamed verify (tv_v2_stream_begin): one column of a window of n pieces -------------
#define TV_KERNEL_V2_STREAM 32    // tv_last_kernel id of a v2 stream (tv_v2_column_kernel + the window's levels + finish)
#define TV_V2_COL_MAX_LOGC 12     // a column is at most 64 MiB (one ring slot): 4,096 leaves, 16 tiles of 256
// Row j of the chunk buffer (data + j * stride) holds bytes [col << (14 + logc), ...) of window piece j: the c = 1 << logc
// leaves col * c .. col * c + c - 1 of its tree, an aligned subtree.  The kernel hashes the leaves (a position inside
// the tree but past piece_bytes[j] is a zero hash and reads no memory) and reduces them in LDS to ONE node, the
// subtree's root at level min(logc, log2 tree_leaves[j]), stored at node slot (j << logn) + col of `nodes`
// (SoA [8][n << logn], big-endian values): level buffer A of the window's top tree, whose row of piece j is
// max(1, tree_leaves[j] >> logc) nodes wide.  A piece whose tree does not reach the column (col * c >= tree_leaves[j])
// writes nothing.
struct TvV2Col {
    const uint8_t* data;
    uint64_t stride;
    uint32_t n;                  // pieces in the window
    uint32_t logc;               // leaves per column = 1 << logc (<= TV_V2_COL_MAX_LOGC)
    uint32_t logn;               // columns per piece = 1 << logn
    uint32_t col;                // this column
    const uint32_t* piece_bytes; // [n]
    const uint32_t* tree_leaves; // [n]
    uint32_t* nodes;             // [8][n << logn]
    uint64_t* clock;             // TV_OPT_CLOCK_PROBE (as TvPieces::clock); null = off
};
hipError_t tv_v2_launch_column(const TvV2Col& p, hipStream_t s, uint32_t* workgroups);

// ---- the v2 block launch (tv_v2_leaf_hashes, tv_v2_check_blocks): m 16 KiB blocks, one lane each, no tree ----------
#define TV_KERNEL_V2_BLOCKS 64    // tv_last_kernel id of tv_v2_leaf_hashes / tv_v2_check_blocks (tv_v2_block_kernel, one launch)
#define TV_V2_BLOCKS_MAX_ITEMS (1u << 22)   // = TV_V2_BLOCKS_MAX of the public header: item indices stay 32-bit
// Item t is the lens[t] (1 .. 16,384) bytes at data + rows[t] * stride + leaves[t] * 16384: block leaves[t] of the
// piece in payload row (or slot) rows[t].  Consecutive items are consecutive blocks of a piece, so a wave reads
// addresses 16 KiB apart (the TV_V2_MAP_LEAF pattern).  check = false: item t's hash words to hashes[q * m + t]
// (q = 0 .. 7, big-endian values).  check = true: they are compared with expect[q * m + t], and bit (t & 63) of
// out64[t >> 6] is set iff all eight match; out64 (ceil(m / 64) words) must be zero before the launch.
struct TvV2Blocks {
    const uint8_t* data;
    uint64_t stride;
    uint32_t m;                  // items (<= TV_V2_BLOCKS_MAX_ITEMS)
    const uint32_t* rows;        // [m]
    const uint32_t* leaves;      // [m]
    const uint32_t* lens;        // [m]
    const uint32_t* expect;      // check: [8][m]
    uint32_t* hashes;            // !check: [8][m]
    uint64_t* out64;             // check: [ceil(m / 64)]
};
hipError_t tv_v2_launch_blocks(const TvV2Blocks& p, bool check, hipStream_t s, uint32_t* workgroups);

// ---- hybrid torrents (tv_hybrid.hip): the pad kernel, then the SHA-1 launch and the v2 launch set over the same rows --
#define TV_KERNEL_HYBRID 128      // tv_last_kernel id of tv_hybrid_verify / tv_hybrid_hash
#define TV_KERNEL_HYBRID_STREAM 256   // ... of a hybrid stream (per unit: column pad, SHA-1 column, v2 column launches)
#define TV_KERNEL_HYBRID_LIST 512     // ... of tv_hybrid_verify_list (list pad, SHA-1 list, v2 list launches)

// workgroups (optional): set to the launch's grid size, companions included.
hipError_t tv_launch_verify(const TvPieces& p, int kernel, bool hash, hipStream_t s, int split_pairs = 0,
                            uint32_t* workgroups = nullptr);
hipError_t tv_launch_verify_list(const TvPieces& p, int kernel, hipStream_t s, uint32_t* workgroups = nullptr);
// The batch launch: p.n positions described by b_off / b_len / b_col, groups of tv_batch_span(kernel) by b_geom;
// results through out_bytes as in list mode.
inline uint32_t tv_batch_span(int kernel) { return kernel == TV_KERNEL_TWIN ? 32u : 64u; }
hipError_t tv_launch_verify_batch(const TvPieces& p, int kernel, hipStream_t s, uint32_t* workgroups = nullptr);
hipError_t tv_launch_fill(uint8_t* payload, uint64_t stride, uint64_t first, uint32_t n, uint64_t L,
                          uint64_t seed, hipStream_t s);
// Windowed layouts: bit j of out64 (MSB-first bytes in 64-bit words, as the verify kernels write it) = the
// digest hash[.][j] equals digests[.][j] ([5][dcount] SoA) and avail64 bit j (null: all); j < n, the rest 0.
hipError_t tv_launch_compare(const uint32_t* hash, const uint32_t* digests, uint32_t dcount, uint32_t n,
                             const uint64_t* avail64, uint64_t* out64, hipStream_t s);
