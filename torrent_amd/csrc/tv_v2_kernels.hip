// tv_v2_kernels.hip -- gfx950 kernels of the BitTorrent v2 (BEP 52) path: SHA-256 merkle piece roots.
//
// A v2 piece hash is the root of a binary SHA-256 tree over the piece's 16 KiB blocks ("leaves"):
//   leaf      = SHA-256 of the block at its real length (a file's last block is 1 .. 16,384 bytes, never padded);
//   interior  = SHA-256(left || right), a 64-byte message: two compressions, the second over a constant block;
//   a leaf position past the file's end is 32 zero bytes (not the hash of anything); the nodes above it are hashed
//   like any other.
// The serial unit is therefore 16 KiB, not a piece, so the parallelism is pieces x leaves:
//   leaf kernel   : one lane per leaf; each lane loads its own 64-byte blocks (register prefetch, 3 blocks ahead, as
//                   the SHA-1 lane kernel) and runs the compression in plain C++ (tv_sha256.h).  Leaf hashes go to the
//                   node buffer A, SoA [8][pieces x W], W = L / 16 KiB.
//   level kernel  : one launch per tree level, one lane per parent node; the levels ping-pong between A and B.
//   finish kernel : one lane per piece: the root against the expected hash and the availability bit -> MSB-first
//                   bitfield words (as tv_compare_kernel), or the root out (creation mode).
//   list kernel   : tv_v2_verify_list's single launch: the leaf hashing above, then the piece's tree levels in LDS
//                   inside the workgroup, root against the entry's expected hash -> one byte per entry.
//   column kernel : a streamed verify's unit (tv_v2_stream_begin): a column of every piece of a window is a whole aligned
//                   subtree of each piece, hashed and reduced in LDS to one node per piece; the level and finish
//                   kernels then run over those nodes.
//   block kernel  : tv_v2_leaf_hashes / tv_v2_check_blocks: one lane per listed 16 KiB block (no tree): its hash out,
//                   or against the expected leaf hash -> one ballot word per wave.
// Which lane hashes which leaf (TvV2::map): consecutive leaves of a piece (addresses 16 KiB apart), or one leaf index
// of 64 consecutive pieces (addresses `stride` apart, the layout the SHA-1 lane kernel reads).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tv_block.h"
#include "tv_internal.h"
#include "tv_sha256.h"

namespace {

constexpr uint32_t kLeaf = 16384;
constexpr int kDepth = 3;   // raw blocks in flight per lane (the SHA-1 lane kernel's TV_LANE_DEPTH)

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o < v ? o : v;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o > v ? o : v;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ void bswap_block(const uint4 (&r)[4], uint32_t w[16]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w[4 * i + 0] = bswap32(r[i].x);
        w[4 * i + 1] = bswap32(r[i].y);
        w[4 * i + 2] = bswap32(r[i].z);
        w[4 * i + 3] = bswap32(r[i].w);
    }
}

// SHA-256 of the `len` (1 .. 16,384) bytes at `leaf` into h, for the lanes with `active` set; the other lanes of the
// wave hash nothing and get no h.  EVERY lane of the wave calls it (the block ranges below are wave reductions).
// Raw blocks load kDepth ahead into registers (load_block); the padded tail goes through build_tail_block.
__device__ __forceinline__ void hash_leaf(const uint8_t* leaf, uint32_t len, bool active, uint32_t h[8]) {
    // wave-uniform block ranges over the wave's hashing lanes: [0, fast_end) are raw data for every one of them,
    // [fast_end, end) go the padded-block way with the lanes past their last block masked
    const uint32_t nb = active ? (uint32_t)nblocks(len) : 0;
    const uint32_t fast_end = wave_min(active ? len >> 6 : 0xFFFFFFFFu);
    const uint32_t end = wave_max(nb);
    if (active) {
        uint32_t w[16];
        tv256::iv(h);
        uint32_t b = 0;
        if (b < fast_end) {
            // loads are unconditional (the block index is clamped to the last raw block), so they are never
            // predicated and stay in flight across a block
            const uint32_t last = fast_end - 1;
            uint4 R[kDepth][4];
#pragma unroll
            for (int d = 0; d < kDepth; d++) load_block(leaf, b + d < last ? b + d : last, R[d]);
            for (;;) {
#pragma unroll
                for (int d = 0; d < kDepth; d++) {
                    bswap_block(R[d], w);
                    load_block(leaf, b + kDepth < last ? b + kDepth : last, R[d]);
                    tv256::compress(h, w, h);
                    if (++b >= fast_end) goto raw_done;
                }
            }
        }
    raw_done:
        for (; b < end; b++) {
            build_tail_block(leaf, len, b, w);
            uint32_t r[8];
            tv256::compress(h, w, r);
            if (b < nb) {
#pragma unroll
                for (int i = 0; i < 8; i++) h[i] = r[i];
            }
        }
    }
}

// An interior node: h = SHA-256(left || right), the 16 words of the two children in w (consumed).
__device__ __forceinline__ void hash_pair(uint32_t w[16], uint32_t h[8]) {
    tv256::iv(h);
    tv256::compress(h, w, h);
    uint32_t pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512u};   // a 64-byte message's padding
    tv256::compress(h, pad, h);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// leaf kernel: lane t of the launch hashes leaf k of piece j (MAP decides which).
// ------------------------------------------------------------------------------------------
template <int MAP>
__global__ __launch_bounds__(256) void tv_v2_leaf_kernel(TvV2 p) {
    uint64_t t0 = 0, r0 = 0;
    if (p.clock && blockIdx.x == 0) {   // clock probe, as the SHA-1 kernels' ClockStamp
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
    }
    const uint32_t logW = p.logW, W = 1u << logW;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint64_t j;
    uint32_t k;
    if (MAP == TV_V2_MAP_LEAF) {
        j = t >> logW;
        k = (uint32_t)t & (W - 1u);
    } else {   // groups of 64 pieces; inside a group lane = piece, wave = leaf index
        const uint32_t r = (uint32_t)t & ((64u << logW) - 1u);
        j = (t >> (6u + logW)) * 64u + (r & 63u);
        k = r >> 6;
    }
    const bool valid = j < p.n;
    const uint64_t bytes = valid ? p.piece_bytes[j] : 0;
    const uint32_t wj = valid ? p.tree_leaves[j] : 0;
    const bool in_tree = k < wj;
    const uint64_t lo = (uint64_t)k * kLeaf;
    const bool active = in_tree && lo < bytes;            // the leaf holds >= 1 valid byte
    const uint32_t len = active ? (uint32_t)(bytes - lo < kLeaf ? bytes - lo : kLeaf) : 0;
    const uint64_t np = (uint64_t)p.n << logW;            // SoA row length of A
    const uint64_t slot = (j << logW) + k;
    if (in_tree && !active) {   // a padding leaf: a zero hash, and no memory read
#pragma unroll
        for (int q = 0; q < 8; q++) p.nodes_a[q * np + slot] = 0;
    }
    uint32_t h[8];
    hash_leaf(p.data + j * p.stride + lo, len, active, h);
    if (active) {
#pragma unroll
        for (int q = 0; q < 8; q++) p.nodes_a[q * np + slot] = h[q];
    }
    if (p.clock && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        reinterpret_cast<ulonglong2*>(p.clock)[0] = make_ulonglong2(t0, r0);
        reinterpret_cast<ulonglong2*>(p.clock)[1] = make_ulonglong2(t1, r1);
    }
}

// ------------------------------------------------------------------------------------------
// level kernel: parent i of piece j at tree level `level` = SHA-256(child 2i || child 2i + 1).  log_half = log2 of the
// lanes per piece in this launch (the widest tree's parents at this level); a piece with a narrower tree uses fewer.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tv_v2_level_kernel(TvV2 p, uint32_t level, uint32_t log_half) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t j = t >> log_half;
    const uint32_t i = (uint32_t)t & ((1u << log_half) - 1u);
    if (j >= p.n) return;
    if (i >= (p.tree_leaves[j] >> (level + 1u))) return;
    const uint64_t W = 1ull << p.logW, WB = W > 1 ? W / 2 : 1;
    const bool from_a = (level & 1u) == 0;
    const uint32_t* in = from_a ? p.nodes_a : p.nodes_b;
    uint32_t* out = from_a ? p.nodes_b : p.nodes_a;
    const uint64_t in_row = from_a ? W : WB, out_row = from_a ? WB : W;
    const uint64_t in_np = p.n * in_row, out_np = p.n * out_row;
    const uint64_t src = j * in_row + 2ull * i, dst = j * out_row + i;   // (in_row and src are even: 8-byte loads)
    uint32_t w[16], h[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint2 v = *reinterpret_cast<const uint2*>(in + q * in_np + src);
        w[q] = v.x;       // word q of the left child
        w[8 + q] = v.y;   // word q of the right child
    }
    tv256::iv(h);
    tv256::compress(h, w, h);
    uint32_t pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512u};   // a 64-byte message's padding
    tv256::compress(h, pad, h);
#pragma unroll
    for (int q = 0; q < 8; q++) out[q * out_np + dst] = h[q];
}

// ------------------------------------------------------------------------------------------
// finish kernel: piece j's root (node 0 of its row in A after an even number of levels, in B after an odd one).
// ------------------------------------------------------------------------------------------
template <bool HASH>
__global__ __launch_bounds__(256) void tv_v2_finish_kernel(TvV2 p) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    bool ok = j < p.n;
    if (ok) {
        const uint64_t W = 1ull << p.logW, WB = W > 1 ? W / 2 : 1;
        const uint32_t lw = 31u - (uint32_t)__builtin_clz(p.tree_leaves[j]);
        const bool in_a = (lw & 1u) == 0;
        const uint32_t* src = in_a ? p.nodes_a : p.nodes_b;
        const uint64_t row = in_a ? W : WB, np = p.n * row;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t v = src[q * np + j * row];
            if (HASH) p.roots[(uint64_t)q * p.n + j] = v;
            else ok &= v == p.expect[(uint64_t)q * p.n + j];
        }
    }
    if (HASH) return;
    const uint64_t mask = __ballot(ok);
    // lane 0 of the wave: pieces j .. j + 63, word j >> 6 (a streamed window's launch stops at its own words)
    if ((threadIdx.x & 63u) == 0 && (p.out_words == 0 || (j >> 6) < p.out_words)) {
        uint64_t bits = __builtin_bswap64(__builtin_bitreverse64(mask));   // ballot bit l -> MSB-first bytes
        if (p.avail64) bits &= p.avail64[j >> 6];
        p.out64[j >> 6] = bits;
    }
}

// ------------------------------------------------------------------------------------------
// list kernel (tv_v2_verify_list): a piece's whole tree in one workgroup, its nodes in LDS.
//   W <= 256: a workgroup covers G = 256 / W consecutive list entries, one lane per leaf position (one tile).
//   W  > 256: a workgroup owns one entry and walks it in W / 256 tiles of 256 leaves; each tile is reduced to its
//             subtree root (8 levels), the roots collect in s_root, and that array is reduced at the end.
// A level is compacted: parent t = SHA-256(node 2t || node 2t + 1) of the 256-node row, written back to position t, so
// level l keeps 256 >> (l + 1) consecutive lanes (whole waves) busy.  An entry's root is node 0 of its segment after
// log2(w) levels: the lane that computes it compares it with the expected words and writes out_bytes[e].
// Every loop that holds a barrier runs on logW alone (workgroup-uniform); lanes with no leaf (a padding position, an
// entry past m) skip the hashing, never a barrier, and no lane returns early.
// ------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ void list_emit(const TvV2List& p, uint32_t e, const uint32_t h[8]) {
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; q++) ok &= h[q] == p.expect[(uint64_t)q * p.m + e];
    p.out_bytes[e] = ok ? 1 : 0;
}

// One compacted level of the 256-node row `s`: lanes [0, parents) each hash one pair.  Returns true in those lanes,
// with the parent in h.
__device__ __forceinline__ bool list_level(uint32_t (&s)[8][256], uint32_t t, uint32_t parents, uint32_t h[8]) {
    const bool par = t < parents;
    uint32_t w[16];
    if (par) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint2 v = *reinterpret_cast<const uint2*>(&s[q][2 * t]);
            w[q] = v.x;       // word q of the left child
            w[8 + q] = v.y;   // word q of the right child
        }
    }
    __syncthreads();   // every pair is read before a parent overwrites a child of another lane's pair
    if (par) {
        hash_pair(w, h);
#pragma unroll
        for (int q = 0; q < 8; q++) s[q][t] = h[q];
    }
    __syncthreads();
    return par;
}

}  // namespace

// TILED = W > 256 (the launcher's choice), and only the tile loop depends on it: with the leaf hashing inside a loop the
// compiler hoists the compression's constants out of it and the kernel takes 224 VGPRs (2 waves per SIMD); without
// the loop it takes 126, the leaf kernel's 4 waves per SIMD.
template <bool TILED>
__global__ __launch_bounds__(256) void tv_v2_list_kernel(TvV2List p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_node[8][256];   // the tile's current level, SoA
    __shared__ __attribute__((aligned(16))) uint32_t s_root[8][256];   // W > 256: the tiles' subtree roots (W / 256 <= 256 of them)
    __shared__ uint32_t s_lw[256];        // log2 of the tree width of the workgroup's entry g (0xFF: no entry)
    const uint32_t t = threadIdx.x;
    const uint32_t logW = p.logW, logT = logW < 8u ? logW : 8u;   // a tile holds 1 << logT leaves of an entry
    const uint32_t tiles = 1u << (logW - logT);
    const uint32_t e0 = blockIdx.x << (8u - logT);                // the workgroup's first entry
    const uint32_t e = e0 + (t >> logT), kt = t & ((1u << logT) - 1u);
    const bool valid = e < p.m;
    const uint32_t bytes = valid ? p.bytes[e] : 0;
    const uint32_t we = valid ? p.widths[e] : 0;
    const uint8_t* row = p.data + (valid ? (uint64_t)p.rows[e] * p.stride : 0);
    if (kt == 0) s_lw[t >> logT] = valid ? 31u - (uint32_t)__builtin_clz(we) : 0xFFu;
    uint32_t h[8];
    for (uint32_t T = 0; T < (TILED ? tiles : 1u); T++) {
        const uint32_t k = (T << logT) + kt;
        const uint32_t lo = k * kLeaf;                            // (k < 65,536: below 2^30)
        const bool active = k < we && lo < bytes;                 // the leaf holds >= 1 valid byte
        const uint32_t len = active ? (bytes - lo < kLeaf ? bytes - lo : kLeaf) : 0;
        hash_leaf(row + lo, len, active, h);
        if (!active) {   // a padding leaf (or no entry): a zero hash, and no memory read
#pragma unroll
            for (int q = 0; q < 8; q++) h[q] = 0;
        }
        if (T == 0 && kt == 0 && we == 1) list_emit(p, e, h);     // a one-leaf tree: the leaf is the root
#pragma unroll
        for (int q = 0; q < 8; q++) s_node[q][t] = h[q];
        __syncthreads();
        for (uint32_t l = 0; l < logT; l++) {
            if (!list_level(s_node, t, 256u >> (l + 1u), h)) continue;
            const uint32_t sh = logT - l - 1u, g = t >> sh;       // node t is node (t & mask) of entry g's level l + 1
            if ((t & ((1u << sh) - 1u)) != 0) continue;
            if (T == 0 && s_lw[g] == l + 1u) list_emit(p, e0 + g, h);
            if (tiles > 1 && sh == 0) {                           // (lane 0) the tile's subtree root
#pragma unroll
                for (int q = 0; q < 8; q++) s_root[q][T] = h[q];
            }
        }
    }
    // W > 256: the tile roots' levels 8 .. logW - 1.  Lane 0 stored the last tile's root after that tile's last
    // barrier, and with 256 tiles its reader (lane 127) is in another wave.
    if (TILED) __syncthreads();
    for (uint32_t l = 8; l < logW; l++)
        if (list_level(s_root, t, tiles >> (l - 7u), h) && t == 0 && s_lw[0] == l + 1u) list_emit(p, e0, h);
}

// ------------------------------------------------------------------------------------------
// column kernel (a streamed verify, tv_v2_stream_begin): one column of a window of pieces.  A column of a piece is c
// = 1 << logc consecutive leaves starting at a multiple of c: a whole aligned subtree, so nothing is carried from one
// column to the next -- the workgroup that hashes the leaves reduces them in LDS to the subtree's root (level
// min(logc, log2 w) of a piece whose tree is w leaves wide) and stores that ONE node; the window's top tree over the
// L / C nodes of each piece runs in the level and finish kernels after the last column.
//   c <= 256: a workgroup covers G = 256 / c consecutive rows of the chunk buffer, one lane per leaf (one tile).
//   c  > 256: a workgroup owns one row and walks it in c / 256 tiles, as the list kernel walks a piece.
// A leaf position inside the tree but past the piece's bytes is a zero hash and reads no memory (its row of the chunk
// buffer may hold an earlier window's bytes there, or nothing); a column wholly past the bytes therefore reduces zero
// hashes to the true all-zero subtree root.  A piece whose tree ends before the column stores nothing.
// As in the list kernel, every loop that holds a barrier runs on logc alone and no lane returns early; TILED keeps
// the tile loop out of the one-tile instantiation (its register count: see tv_v2_list_kernel).
// ------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ void column_store(const TvV2Col& p, uint32_t j, const uint32_t h[8]) {
    const uint64_t np = (uint64_t)p.n << p.logn, slot = ((uint64_t)j << p.logn) + p.col;
#pragma unroll
    for (int q = 0; q < 8; q++) p.nodes[q * np + slot] = h[q];
}

}  // namespace

template <bool TILED>
__global__ __launch_bounds__(256) void tv_v2_column_kernel(TvV2Col p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_node[8][256];   // the tile's current level, SoA
    __shared__ __attribute__((aligned(16))) uint32_t s_root[8][256];   // c > 256: the tiles' subtree roots (<= 16 of them)
    __shared__ uint32_t s_tg[256];        // the level at which row g's node is complete (0xFF: no row, or out of reach)
    uint64_t t0 = 0, r0 = 0;
    if (p.clock && blockIdx.x == 0) {   // clock probe, as the leaf kernel's
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
    }
    const uint32_t t = threadIdx.x;
    const uint32_t logc = p.logc, logT = logc < 8u ? logc : 8u;   // a tile holds 1 << logT leaves of a row
    const uint32_t tiles = 1u << (logc - logT);
    const uint32_t j0 = blockIdx.x << (8u - logT);                // the workgroup's first row
    const uint32_t j = j0 + (t >> logT), kt = t & ((1u << logT) - 1u);
    const bool valid = j < p.n;
    const uint32_t bytes = valid ? p.piece_bytes[j] : 0;
    const uint32_t wj = valid ? p.tree_leaves[j] : 0;
    const uint64_t k0 = (uint64_t)p.col << logc;                  // the column's first leaf
    const bool reach = k0 < wj;                                   // the piece's tree reaches this column
    const uint32_t lw = wj ? 31u - (uint32_t)__builtin_clz(wj) : 0u;
    const uint32_t target = lw < logc ? lw : logc;
    const uint8_t* row = p.data + (valid ? (uint64_t)j * p.stride : 0);
    if (kt == 0) s_tg[t >> logT] = reach ? target : 0xFFu;
    uint32_t h[8];
    for (uint32_t T = 0; T < (TILED ? tiles : 1u); T++) {
        const uint32_t kr = (T << logT) + kt;                     // leaf of the column (its 16 KiB of the row)
        const uint64_t lo = (k0 + kr) * kLeaf;                    // ... and its first byte in the piece
        const bool active = k0 + kr < wj && lo < bytes;           // the leaf holds >= 1 valid byte
        const uint32_t len = active ? (uint32_t)(bytes - lo < kLeaf ? bytes - lo : kLeaf) : 0;
        hash_leaf(row + (uint64_t)kr * kLeaf, len, active, h);
        if (!active) {   // a padding leaf (or no row): a zero hash, and no memory read
#pragma unroll
            for (int q = 0; q < 8; q++) h[q] = 0;
        }
        if (T == 0 && kt == 0 && reach && target == 0) column_store(p, j, h);   // c == 1 or a one-leaf tree
#pragma unroll
        for (int q = 0; q < 8; q++) s_node[q][t] = h[q];
        __syncthreads();
        for (uint32_t l = 0; l < logT; l++) {
            if (!list_level(s_node, t, 256u >> (l + 1u), h)) continue;
            const uint32_t sh = logT - l - 1u, g = t >> sh;       // node t is node (t & mask) of row g's level l + 1
            if ((t & ((1u << sh) - 1u)) != 0) continue;
            if (T == 0 && s_tg[g] == l + 1u) column_store(p, j0 + g, h);
            if (tiles > 1 && sh == 0) {                           // (lane 0) the tile's subtree root
#pragma unroll
                for (int q = 0; q < 8; q++) s_root[q][T] = h[q];
            }
        }
    }
    // c > 256: the tile roots' levels 8 .. logc - 1 (lane 0 stored the last tile's root after that tile's last barrier)
    if (TILED) __syncthreads();
    for (uint32_t l = 8; l < logc; l++)
        if (list_level(s_root, t, tiles >> (l - 7u), h) && t == 0 && s_tg[0] == l + 1u) column_store(p, j0, h);
    if (p.clock && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        reinterpret_cast<ulonglong2*>(p.clock)[0] = make_ulonglong2(t0, r0);
        reinterpret_cast<ulonglong2*>(p.clock)[1] = make_ulonglong2(t1, r1);
    }
}

// ------------------------------------------------------------------------------------------
// block kernel (tv_v2_leaf_hashes, tv_v2_check_blocks): the unit is the 16 KiB block, not the piece.  Lane t of the
// launch hashes item t: the lens[t] bytes at row rows[t], leaf leaves[t].  The host lists a piece's blocks in
// ascending order, so the lanes of a wave read addresses 16 KiB apart (the TV_V2_MAP_LEAF pattern).  No LDS, no tree
// and no loop around hash_leaf: the one-tile kernels' register shape (see tv_v2_list_kernel).  Lanes past m call
// hash_leaf inactive (its block ranges are wave reductions) and no lane returns before it.
//   CHECK = false: the item's eight hash words out.
//   CHECK = true : the words against the item's expected ones; lane 0 of each wave stores the wave's ballot (bit l =
//                  item 64 * wave + l matches).  The host zeroes out64 before the launch: an item the launch does
//                  not reach reads as a mismatch.
// ------------------------------------------------------------------------------------------
template <bool CHECK>
__global__ __launch_bounds__(256) void tv_v2_block_kernel(TvV2Blocks p) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;       // (m <= 2^22)
    const bool active = t < p.m;
    const uint32_t row = active ? p.rows[t] : 0;
    const uint32_t leaf = active ? p.leaves[t] : 0;
    const uint32_t len = active ? p.lens[t] : 0;
    uint32_t h[8];
    hash_leaf(p.data + (uint64_t)row * p.stride + (uint64_t)leaf * kLeaf, len, active, h);
    if (CHECK) {
        bool ok = active;
        if (active) {
#pragma unroll
            for (int q = 0; q < 8; q++) ok &= h[q] == p.expect[(uint64_t)q * p.m + t];
        }
        const uint64_t mask = __ballot(ok);
        if ((threadIdx.x & 63u) == 0 && active) p.out64[t >> 6] = mask;
    } else if (active) {
#pragma unroll
        for (int q = 0; q < 8; q++) p.hashes[(uint64_t)q * p.m + t] = h[q];
    }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (tv_v2.hip)
// ------------------------------------------------------------------------------------------
hipError_t tv_v2_launch_blocks(const TvV2Blocks& p, bool check, hipStream_t s, uint32_t* workgroups) {
    if (workgroups) *workgroups = 0;
    if (p.m == 0) return hipSuccess;
    if (p.m > TV_V2_BLOCKS_MAX_ITEMS) return hipErrorInvalidValue;
    const uint32_t grid = (p.m + 255u) / 256u;
    if (workgroups) *workgroups = grid;
    if (check) hipLaunchKernelGGL(tv_v2_block_kernel<true>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(tv_v2_block_kernel<false>, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t tv_v2_launch_column(const TvV2Col& p, hipStream_t s, uint32_t* workgroups) {
    if (workgroups) *workgroups = 0;
    if (p.n == 0) return hipSuccess;
    if (p.logc > TV_V2_COL_MAX_LOGC || (p.col >> p.logn) != 0) return hipErrorInvalidValue;
    const uint32_t logG = p.logc < 8u ? 8u - p.logc : 0u;   // rows per workgroup: max(1, 256 / c)
    const uint64_t grid = (((uint64_t)p.n - 1) >> logG) + 1;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (workgroups) *workgroups = (uint32_t)grid;
    if (p.logc > 8u) hipLaunchKernelGGL(tv_v2_column_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(tv_v2_column_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t tv_v2_launch_leaves(const TvV2& p, hipStream_t s, uint32_t* workgroups) {
    if (workgroups) *workgroups = 0;
    if (p.n == 0) return hipSuccess;
    const uint64_t pieces = p.map == TV_V2_MAP_PIECE ? ((uint64_t)p.n + 63) / 64 * 64 : p.n;
    const uint64_t grid = ((pieces << p.logW) + 255) / 256;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (workgroups) *workgroups = (uint32_t)grid;
    if (p.map == TV_V2_MAP_PIECE)
        hipLaunchKernelGGL((tv_v2_leaf_kernel<TV_V2_MAP_PIECE>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((tv_v2_leaf_kernel<TV_V2_MAP_LEAF>), dim3((unsigned)grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t tv_v2_launch_level(const TvV2& p, uint32_t level, uint32_t maxlog, hipStream_t s) {
    if (p.n == 0 || level >= maxlog) return hipSuccess;
    const uint32_t log_half = maxlog - level - 1;
    const uint64_t grid = (((uint64_t)p.n << log_half) + 255) / 256;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(tv_v2_level_kernel, dim3((unsigned)grid), dim3(256), 0, s, p, level, log_half);
    return hipGetLastError();
}

hipError_t tv_v2_launch_list(const TvV2List& p, hipStream_t s, uint32_t* workgroups) {
    if (workgroups) *workgroups = 0;
    if (p.m == 0) return hipSuccess;
    if (p.logW > TV_V2_LIST_MAX_LOGW) return hipErrorInvalidValue;
    const uint32_t logG = p.logW < 8u ? 8u - p.logW : 0u;   // entries per workgroup: max(1, 256 / W)
    const uint64_t grid = (((uint64_t)p.m - 1) >> logG) + 1;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (workgroups) *workgroups = (uint32_t)grid;
    if (p.logW > 8u) hipLaunchKernelGGL(tv_v2_list_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(tv_v2_list_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t tv_v2_launch_finish(const TvV2& p, bool hash, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    const dim3 grid((p.n + 255) / 256);
    if (hash) hipLaunchKernelGGL((tv_v2_finish_kernel<true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((tv_v2_finish_kernel<false>), grid, dim3(256), 0, s, p);
    return hipGetLastError();
}
