// tv_kernels.hip -- gfx950 SHA-1 piece-verification kernels.
//
// Reference semantics (rclarey/torrent): piece i = bytes [i*L, i*L + len_i) of the linear
// torrent space (torrent.ts:165,186); len_i per piece.ts:16-19; digest = SHA-1 as in
// crypto.subtle.digest("SHA-1", content) (tools/make_torrent.ts:28-31); have-bit i set iff
// the digest equals info.pieces[i] (metainfo.ts:111) and the bytes were readable
// (Storage.get non-null, storage.ts:50-65), MSB-first (torrent.ts:147-149).
//
// SHA-1 is serial inside a piece, so parallelism comes from pieces only.  Three kernels (plus list and batch modes):
//   lane  : one lane per piece; each lane loads its own 64-byte blocks (register prefetch, TV_LANE_DEPTH = 3
//           blocks ahead) and runs the full compression (schedule + rounds) as one generated asm block
//           (613 VALU per block).  For > 32,768 pieces per GPU, where every SIMD has a wave.
//   split : schedule offload.  A workgroup is PAIRS x (rounds, helper) waves, 64 pieces per pair: a helper
//           loads the blocks and writes K+W[0..79] into a 3-buffer LDS ring two blocks ahead (generated asm:
//           v_perm bswap, v_bitop3 xor3, K adds, ds_write_b128); the rounds wave runs only the 80 rounds
//           from LDS (405 VALU + 20 ds_read_b128 + 5 waits per block).  A lone wave issues one VALU per
//           ~4.07 cycles (tools/ubench_fetch.hip), so with fewer pieces than SIMDs the per-lane
//           instruction count IS the bound; this cuts the serial stream from 613 to 405 VALU per block.
//           For 16,384 < pieces <= 32,768 per GPU.
//   twin  : split with TWO lanes per piece: of every two rounds one lane of the pair computes the first and the
//           other the second, sharing F and `F + e + KW` and passing rotl5-and-add to each other by DPP (367
//           VALU per block); each lane reads only the K+W quads of its parity (10 ds_read_b128 per block), and
//           a two-lane helper expands the schedule by parity.  For <= 16,384 pieces per GPU (every wave still
//           has a SIMD to itself).
// What the kernels share is written once: resolve_group() turns a group of a launch into each lane's piece, block
// range and bytes (resident, list and batch mode); helper_wave() / rounds_wave() are the two wave bodies of split and twin,
// with the barrier protocol stated above them; finish() / finish_list() write the results.  The generated blocks
// and loops are in sha1_asm.h (tools/gen_sha1_asm.py).
//
// HBM layout: resident piece j (shard-local) starts at payload + j*stride, stride = L + pad
// (pad breaks the power-of-two stride that would put all 64 lanes of a wave on one channel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sha1_asm.h"
#include "tv_block.h"
#include "tv_internal.h"

#define TV_K0 0x5A827999u
#define TV_K1 0x6ED9EBA1u
#define TV_K2 0x8F1BBCDCu
#define TV_K3 0xCA62C1D6u

namespace {

__device__ __forceinline__ void sha1_iv(uint32_t h[5]) {
    h[0] = 0x67452301u; h[1] = 0xEFCDAB89u; h[2] = 0x98BADCFEu; h[3] = 0x10325476u; h[4] = 0xC3D2E1F0u;
}

// Per-group uniform geometry.  Every piece of a launch has length L except the global last
// piece (launch-local index last_idx), which is always the final piece of the launch.  All
// values are made provably wave-uniform (readfirstlane) so loop control stays scalar and the
// prefetch loads are never predicated (a predicated load forces a vmcnt(0) + copy at the join).
struct WaveGeom {
    uint32_t fast_begin;  // first block of this launch
    uint32_t fast_end;    // blocks [fast_begin, fast_end) are raw data for EVERY lane of the group
    uint32_t end;         // blocks [.., end) are processed (max over lanes, clipped to blk_end)
    uint32_t nb_min;      // every lane has at least nb_min blocks (no masking below it)
};

__device__ __forceinline__ uint32_t uni(uint64_t x) {
    return __builtin_amdgcn_readfirstlane((uint32_t)x);
}

// has_last: some lane's piece is the last piece; only_last: every lane's is.
__device__ __forceinline__ WaveGeom wave_geom(const TvPieces& p, bool has_last, bool only_last) {
    const uint64_t nfull_min = (has_last ? p.last_len : p.L) / 64;
    const uint64_t nb_max = nblocks(only_last ? p.last_len : p.L);
    const uint64_t nb_min = nblocks(has_last ? p.last_len : p.L);
    WaveGeom g;
    g.fast_begin = uni(p.blk_begin);
    g.fast_end = uni(nfull_min < p.blk_end ? nfull_min : p.blk_end);
    g.end = uni(nb_max < p.blk_end ? nb_max : p.blk_end);
    g.nb_min = uni(nb_min);
    return g;
}

// A main group [g0, g0 + span) has the (full-length) last piece iff last_idx falls inside it; the clamped lanes after
// it hash it too, so it is the group's only piece iff it is the first.
__device__ __forceinline__ WaveGeom main_geom(const TvPieces& p, uint32_t g0, uint32_t span) {
    const bool has_last = p.last_idx < p.n_main && p.last_idx >= g0 && p.last_idx - g0 < span;
    return wave_geom(p, has_last, has_last && p.last_idx == g0);
}

// A GROUP is the `span` consecutive entries of a launch that must agree on block counts: a wave of the lane and
// list kernels (64), a split workgroup (64 per pair), a twin workgroup (32 per pair).  Main groups cover entries
// [0, n_main); a SHORT last piece (n_main < n) is never in a main group but gets the group after them to itself,
// whose every lane hashes it, so that no main group runs its short tail.  This is one lane's view of its group.
// (lane_group spells the resident case of resolve_group() out in place: behind the call the compiler lays the
// prologue out differently, which moves the raw-block loop in its 64-byte lines, measured -0.5 % at 16,384 pieces.)
struct Group {
    bool last_grp;         // (uniform) the short last piece's own group
    uint32_t g0;           // first entry of a main group
    uint32_t j;            // this lane's entry, NOT clamped: the lane owns outputs only if j < n_main (list: j < n)
    uint32_t jj;           // the shard piece it hashes: index of its digest, chaining state and availability bit
    WaveGeom g;
    uint64_t len;          // piece jj's length and block count
    uint32_t nb;
    const uint8_t* piece;  // piece jj's byte 0
};

// Group gi (uniform) of a launch, for the lane that runs entry gi * span + off of it.  Lanes past the launch's end
// are clamped to its last main entry: they run the same blocks and write nothing.
// LIST = incremental verify (tv_verify_list): entry j is shard piece idx[j], whose bytes sit in payload row rows[j]
// when the payload is a slot pool (TV_OPT_LIST_SLOTS).  There is no last group: the last piece may sit in any
// lane, so the geometry comes from the wave's ballots (the host puts the last piece's entries in groups of their
// own; waves that must agree, a helper and its rounds wave, see the same entries, so their ballots agree).
// BATCH = many torrents in one launch (tv_batch_verify): entry j is a whole piece of its own length b_len[j] at
// data + b_off[j], its digest in column b_col[j].  The group's block ranges are the host's (b_geom[gi], tv_plan.h
// batch_plan: fast_end * 64 <= every member's length), indexed by the group alone and kept scalar, so every wave of a
// workgroup runs the same loop bounds; lengths, padding and the digest-update mask stay per lane.
enum GroupMode : int { RESIDENT = 0, LIST = 1, BATCH = 2 };

template <int MODE>
__device__ __forceinline__ Group resolve_group(const TvPieces& p, uint32_t gi, uint32_t span, uint32_t off) {
    Group q;
    if constexpr (MODE == BATCH) {
        q.last_grp = false;
        q.g0 = gi * span;
        q.j = q.g0 + off;
        const uint32_t jl = q.j < p.n ? q.j : p.n - 1;   // (the last group's spare lanes: its last entry, a member)
        q.jj = p.b_col[jl];
        const TvBatchGeom r = p.b_geom[gi];
        q.g.fast_begin = 0;
        q.g.fast_end = uni(r.fast_end);
        q.g.end = uni(r.end);
        q.g.nb_min = uni(r.nb_min);
        q.len = p.b_len[jl];
        q.nb = (uint32_t)nblocks(q.len);
        q.piece = p.data + p.b_off[jl];
        return q;
    }
    constexpr bool listed = MODE == LIST;
    const uint32_t nlim = listed ? p.n : p.n_main;
    q.last_grp = !listed && gi >= (nlim + span - 1) / span;
    q.g0 = gi * span;
    q.j = q.last_grp ? p.last_idx : q.g0 + off;
    const uint32_t jl = q.last_grp ? p.last_idx : (q.j < nlim ? q.j : nlim - 1);
    q.jj = listed ? p.idx[jl] : jl;
    const bool is_last = q.jj == p.last_idx;
    q.g = listed ? wave_geom(p, __ballot(is_last) != 0, __ballot(!is_last) == 0)
                 : q.last_grp ? wave_geom(p, true, true) : main_geom(p, q.g0, span);
    q.len = is_last ? p.last_len : p.L;
    q.nb = (uint32_t)nblocks(q.len);
    const uint32_t row = (listed && p.rows) ? p.rows[jl] : q.jj;
    // a list launch always covers whole resident pieces (tv_core.hip resident_launch: data_off = 0, every block),
    // so list mode reads neither data_off nor, in start_state(), a chaining state
    q.piece = p.data + (uint64_t)row * p.stride - (listed ? 0 : p.data_off);
    return q;
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

__device__ __forceinline__ void compress_full(uint32_t h[5], uint32_t w[16]) {
    uint32_t r[5];
    tv_sha1_full(h, r, w, TV_K0, TV_K1, TV_K2, TV_K3);
#pragma unroll
    for (int i = 0; i < 5; i++) h[i] += r[i];
}

// Final step of every resident-mode wave: compare (verify) or store (hash) the digest, or keep the
// chaining value for the next launch of a streamed run.  `writer`: this lane owns piece jj's outputs
// (a main-group lane below n_main, or lane 0 of the short last piece's dedicated group).  Bitfield
// words are OR-ed into the zeroed output (the last group may share a word with a main group).
// j0 = the wave's first piece.  TWIN: lane 16r + k, k < 8, (and its partner 8 lanes up) holds piece j0 + 8r + k,
// j0 a multiple of 32.
template <bool HASH, bool TWIN = false>
__device__ __forceinline__ void finish(const TvPieces& p, bool writer, uint32_t jj, uint32_t j0,
                                       const uint32_t h[5], bool last_grp) {
    if (!p.finalize) {
        if (writer) {
#pragma unroll
            for (int k = 0; k < 5; k++) p.state[(uint64_t)k * p.dcount + jj] = h[k];   // the next column's launch reads it
        }
        return;
    }
    if (HASH) {
        if (writer) {
#pragma unroll
            for (int k = 0; k < 5; k++) p.out_digests[(uint64_t)k * p.dcount + jj] = h[k];
        }
        return;
    }
    bool ok = writer;
#pragma unroll
    for (int k = 0; k < 5; k++) ok &= (h[k] == p.digests[(uint64_t)k * p.dcount + jj]);
    uint64_t mask = __ballot(ok);
    if ((threadIdx.x & 63) == 0) {
        if (TWIN && !last_grp) {   // the role-0 lanes' bytes -> bits 0..31, then to the wave's half of its word
            mask &= 0x00FF00FF00FF00FFull;
            mask = (mask | (mask >> 8)) & 0x0000FFFF0000FFFFull;
            mask = (mask | (mask >> 16)) & 0x00000000FFFFFFFFull;
            mask <<= j0 & 63;
        }
        // mask bit l = piece (j0 & ~63) + l  ->  MSB-first bytes: byte m holds pieces 8m .. 8m+7 of the word
        const uint32_t w = (last_grp ? jj : j0) >> 6;
        uint64_t bits = last_grp ? ((mask & 1) ? 1ull << (((jj >> 3) & 7) * 8 + 7 - (jj & 7)) : 0)
                                 : __builtin_bswap64(__builtin_bitreverse64(mask));
        if (p.avail64) bits &= p.avail64[w];
        if (bits) atomicOr(reinterpret_cast<unsigned long long*>(p.out64 + w), (unsigned long long)bits);
    }
}

// Final step of every list-mode wave: out_bytes[j] = 1 iff entry j's piece jj is available and its digest matches.
__device__ __forceinline__ void finish_list(const TvPieces& p, bool writer, uint32_t j, uint32_t jj,
                                            const uint32_t h[5]) {
    if (!writer) return;
    // (availability: MSB-first bitfield bytes held in little-endian 64-bit words)
    bool ok = p.avail64 ? (p.avail64[jj >> 6] >> (((jj >> 3) & 7) * 8 + (7 - (jj & 7)))) & 1 : true;
#pragma unroll
    for (int k = 0; k < 5; k++) ok &= (h[k] == p.digests[(uint64_t)k * p.dcount + jj]);
    p.out_bytes[j] = ok ? 1 : 0;
}

// Clock probe (TV_OPT_CLOCK_PROBE): workgroup 0 reads the shader clock counter (s_memtime) and the 100 MHz
// real-time counter (s_memrealtime) when it starts; lane 0 of its first (rounds) wave writes both pairs with a
// vector store when it ends.  The ratio of the two intervals is the shader clock the kernel actually ran at.
struct ClockStamp {
    uint64_t t0 = 0, r0 = 0;
    __device__ __forceinline__ void start(const TvPieces& p) {
        if (p.clock && blockIdx.x == 0) {   // (kernel argument and block index: a scalar branch)
            t0 = __builtin_amdgcn_s_memtime();
            r0 = __builtin_amdgcn_s_memrealtime();
        }
    }
    __device__ __forceinline__ void end(const TvPieces& p) const {
        if (p.clock && blockIdx.x == 0 && threadIdx.x == 0) {
            const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
            reinterpret_cast<ulonglong2*>(p.clock)[0] = make_ulonglong2(t0, r0);
            reinterpret_cast<ulonglong2*>(p.clock)[1] = make_ulonglong2(t1, r1);
        }
    }
};

// The chaining value a piece starts this launch with (list mode: always whole pieces, see resolve_group).
template <bool LIST = false>
__device__ __forceinline__ void start_state(const TvPieces& p, uint32_t jj, uint32_t h[5]) {
    if (LIST || p.blk_begin == 0) {
        sha1_iv(h);
    } else {
#pragma unroll
        for (int k = 0; k < 5; k++) h[k] = p.state[(uint64_t)k * p.dcount + jj];  // the previous column's chaining value
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// lane kernel: one lane per piece, full compression per lane.
// ------------------------------------------------------------------------------------------
#ifndef TV_LANE_DEPTH
#define TV_LANE_DEPTH 3   // raw blocks in flight per lane: 3 is 0.8-1.2 % faster than 2, 4 and 6 no better
                          // (profiles/r02/lane_depth.jsonl; A/B: tools/build_variants.py D_TV_LANE_DEPTH=n)
#endif

// Group gw of a launch (a wave: 64 pieces, see resolve_group).  Blocks [blk_begin, blk_end) of p.
// PAIRS: the raw-block loop's register ring holds 4 blocks refilled two at a time, so a lane's two 64-B blocks of
// one 128-B line are requested back to back.  With >= 1 wave per SIMD (>= 65,536 pieces on 256 CUs) the single
// loads of the 3-deep ring let ~2 % of the lines be evicted between their two halves (HBM reads 1.023 x payload
// at 262,144 x 64 KiB, L2 hit 35 %); pairs read 1.0004 x and run 0.3-2.6 % faster there, but 0.4-0.8 % slower
// below one wave per SIMD (profiles/r04/variants/ab_lane_pairs_sweep.jsonl), so the host picks (lane_pairs).
template <bool HASH, bool PAIRS>
__device__ __forceinline__ void lane_group(const TvPieces& p, uint32_t gw) {
    const uint32_t lane = threadIdx.x & 63u;
    // (the grid is whole 4-wave workgroups: the waves past the last group, short last piece's included, have no piece)
    const uint32_t nw_main = (p.n_main + 63u) / 64u;
    const bool last_grp = gw >= nw_main;
    if (last_grp && (gw > nw_main || p.n_main == p.n)) return;  // wave-uniform
    // resolve_group<false>(p, gw, 64, lane), in place (see struct Group)
    const uint32_t j0 = last_grp ? p.last_idx : gw * 64u;
    const uint32_t j = last_grp ? p.last_idx : j0 + lane;
    const uint32_t jj = last_grp ? p.last_idx : (j < p.n_main ? j : p.n_main - 1);
    const bool writer = last_grp ? lane == 0 : j < p.n_main;
    const WaveGeom g = last_grp ? wave_geom(p, true, true) : main_geom(p, j0, 64u);
    const uint64_t len = jj == p.last_idx ? p.last_len : p.L;
    const uint32_t nb = (uint32_t)nblocks(len);
    const uint8_t* piece = p.data + (uint64_t)jj * p.stride - p.data_off;

    uint32_t h[5];
    start_state(p, jj, h);

    uint32_t b = g.fast_begin;
    uint32_t w[16];
    if (PAIRS && b < g.fast_end) {
        // a ring of 4 register blocks refilled in pairs: a lane's two 64-B blocks of one 128-B line are loaded
        // back to back, so both halves reach L2 together
        const uint32_t last = g.fast_end - 1;
        uint4 R[4][4];
#pragma unroll
        for (int d = 0; d < 4; d++) load_block(piece, b + d < last ? b + d : last, R[d]);
        for (;;) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                bswap_block(R[2 * q], w);
                compress_full(h, w);
                if (++b >= g.fast_end) goto raw_done;
                bswap_block(R[2 * q + 1], w);
                load_block(piece, b + 3 < last ? b + 3 : last, R[2 * q]);
                load_block(piece, b + 4 < last ? b + 4 : last, R[2 * q + 1]);
                compress_full(h, w);
                if (++b >= g.fast_end) goto raw_done;
            }
        }
    }
    if (!PAIRS && b < g.fast_end) {
        // TV_LANE_DEPTH register blocks in flight.  Loads are unconditional (the block index is clamped
        // to the last raw block), so they are never predicated and stay in flight across a block.
        constexpr int D = TV_LANE_DEPTH;
        const uint32_t last = g.fast_end - 1;
        uint4 R[D][4];
#pragma unroll
        for (int d = 0; d < D; d++) load_block(piece, b + d < last ? b + d : last, R[d]);
        for (;;) {
#pragma unroll
            for (int d = 0; d < D; d++) {
                bswap_block(R[d], w);
                load_block(piece, b + D < last ? b + D : last, R[d]);
                compress_full(h, w);
                if (++b >= g.fast_end) goto raw_done;
            }
        }
    }
raw_done:
    for (; b < g.end; b++) {
        build_tail_block(piece, len, b, w);
        uint32_t r[5];
        tv_sha1_full(h, r, w, TV_K0, TV_K1, TV_K2, TV_K3);
        if (b < nb) {
#pragma unroll
            for (int i = 0; i < 5; i++) h[i] += r[i];
        }
    }
    finish<HASH>(p, writer, jj, j0, h, last_grp);
}

// TV_LANE_PAD (A/B knob): 64-byte-align the kernel's first instructions, then TV_LANE_PAD 4-byte s_nops, which
// moves the raw-block loop through the 16 word positions of a 64-byte line (tools/build_variants.py D_TV_LANE_PAD)
#define TV_STR2(x) #x
#define TV_STR(x) TV_STR2(x)
template <bool HASH, bool PAIRS>
__global__ __launch_bounds__(256) void tv_lane_kernel(TvPieces p) {
#ifdef TV_LANE_PAD
    asm volatile(".p2align 6\n.rept " TV_STR(TV_LANE_PAD) "\ns_nop 0\n.endr\n" ::: "memory");
#endif
    ClockStamp clk;
    clk.start(p);
    lane_group<HASH, PAIRS>(p, blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    clk.end(p);
}

// ------------------------------------------------------------------------------------------
// schedule offload, shared by the split and twin kernels: a helper wave (loads + message schedule
// into a 3 x 20 KiB LDS ring, two blocks ahead) feeds a rounds wave (80 rounds per block from
// LDS).  One barrier per block.  Then the split kernel.
// ------------------------------------------------------------------------------------------
namespace {

constexpr int kRingWords = 80 * 64;  // one buffer: [20 quads][64 lanes][4 words]
// K+W buffers per pair.  The helper runs TWO blocks ahead (block j lives in buffer j % 3), so a rounds wave
// may read block j + 1 while it runs block j (the twin loop issues those reads mid-block), and the split helper
// need not wait for a block's LDS writes before the next barrier (tools/gen_sha1_asm.py HELPER_WAIT).
constexpr uint32_t kBufs = TV_SHA1_LDS_BUFS;
constexpr uint32_t kAhead = TV_SHA1_HELPER_AHEAD;

__device__ __forceinline__ void lds_barrier() {
    // LDS writes of this wave complete, then the workgroup barrier.  Deliberately NOT
    // __syncthreads(): the helper's global prefetch loads must stay in flight across it.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#if TV_STAMPS
// Diagnostic builds (tools/split_stamps.py; generator TV_GEN_STAMP=1 + -DTV_STAMPS=1): each split wave's asm loop
// time and the cycles its in-loop barriers (and, TV_SHA1_STAMP 2, the helper's vmcnt / lgkmcnt waits) took, per
// workgroup and wave, after the clock probe's 4 words: clock[4 + 8 (4 wg + wave) ..] = {loop cycles, barrier
// cycles, loop blocks, 1, vmcnt-wait cycles, lgkmcnt-wait cycles, 0, 0} (lane 0, vector stores).
static_assert(TV_SHA1_STAMP, "TV_STAMPS needs the generator's TV_GEN_STAMP header");
constexpr uint32_t kStampGroups = 65536;
struct LoopStamp {
    uint32_t bar = 0, vm = 0, lg = 0;
    uint64_t t0 = 0;
    __device__ __forceinline__ void start() { t0 = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void end(const TvPieces& p, uint32_t wave, uint32_t blocks) const {
        const uint64_t t1 = __builtin_amdgcn_s_memtime();
        if (p.clock && blockIdx.x < kStampGroups && (threadIdx.x & 63u) == 0) {
            uint64_t* q = p.clock + 4 + 8 * (4 * (uint64_t)blockIdx.x + wave);
            reinterpret_cast<ulonglong2*>(q)[0] = make_ulonglong2(t1 - t0, bar);
            reinterpret_cast<ulonglong2*>(q)[1] = make_ulonglong2(blocks, 1);
            reinterpret_cast<ulonglong2*>(q)[2] = make_ulonglong2(vm, lg);
        }
    }
};
#endif

// Which generated blocks (sha1_asm.h) a kernel's helper and rounds waves run: all that differs between the split and
// the twin kernel inside the two wave bodies below.  `lds` = the lane's byte address in a ring buffer.  Stamp... =
// the accumulators the loops of a TV_GEN_STAMP header take (none in the shipped build).
struct SplitOps {
    template <typename... Stamp>
    __device__ __forceinline__ void helper_loop(const uint8_t* va, uint32_t nraw, uint32_t lds, Stamp&... st) const {
        tv_sha1_helper_loop(va, nraw, lds, st..., TV_K0, TV_K1, TV_K2, TV_K3);
    }
    __device__ __forceinline__ void schedule_block(const uint32_t w[16], uint32_t lds) const {
        tv_sha1_schedule_lds(w, lds, TV_K0, TV_K1, TV_K2, TV_K3);
    }
    template <typename... Stamp>
    __device__ __forceinline__ void rounds_loop(uint32_t h[5], uint32_t lds, uint32_t nsteps, Stamp&... st) const {
        tv_sha1_rounds_loop(h, lds, nsteps, st..., TV_K0, TV_K1, TV_K2, TV_K3);
    }
    __device__ __forceinline__ void rounds_block(const uint32_t h[5], uint32_t r[5], uint32_t lds) const {
        tv_sha1_lds(h, r, lds, TV_K0, TV_K1, TV_K2, TV_K3);
    }
};
struct TwinOps {
    uint32_t psel;   // the helper lane's v_perm selector: the message words of its parity
    template <typename... Stamp>
    __device__ __forceinline__ void helper_loop(const uint8_t* va, uint32_t nraw, uint32_t lds, Stamp&... st) const {
        tv_sha1_twin_helper_loop(va, nraw, lds, psel, st..., TV_K0, TV_K1, TV_K2, TV_K3);
    }
    __device__ __forceinline__ void schedule_block(const uint32_t w[16], uint32_t lds) const {
        tv_sha1_twin_schedule_lds(w, lds, psel, TV_K0, TV_K1, TV_K2, TV_K3);
    }
    template <typename... Stamp>
    __device__ __forceinline__ void rounds_loop(uint32_t h[5], uint32_t lds, uint32_t nsteps, Stamp&... st) const {
        tv_sha1_roles_rounds_loop(h, lds, nsteps, st...);
    }
    __device__ __forceinline__ void rounds_block(const uint32_t h[5], uint32_t r[5], uint32_t lds) const {
        tv_sha1_roles_lds(h, r, lds);
    }
};

// THE BARRIER PROTOCOL.  Block b of a group's range [b0, end) lives in ring buffer (b - b0) % kBufs.  The barrier is
// workgroup-wide, and EVERY wave of a workgroup, whatever its role, executes exactly one barrier per b in [b0, end]
// (end included: end - b0 + 1 barriers, the same b0 and end in every wave), or the workgroup hangs:
//   helper : writes blocks b0 .. end (the spare block `end` is never consumed) with a barrier after every write but
//            its first kAhead - 1, and kAhead - 1 closing barriers.  So barrier k follows its write of block
//            b0 + k + kAhead - 1: it runs kAhead blocks ahead.
//   rounds : one barrier before its first block (block b0 is written), then one after each block b0 .. end - 1.
//            Barrier k + 1 says "block b0 + k consumed": the helper's next write, block b0 + k + 1 + kAhead, goes
//            to that buffer (kAhead = kBufs - 1).
//   idle   : one barrier per b in [b0, end].
// The generated loops keep the same count: helper_loop a barrier after every block but the first, rounds_loop one
// after every block.
__device__ __forceinline__ uint32_t ring_buf(uint32_t lds_lane, uint32_t k) {
    return lds_lane + (k % kBufs) * (kRingWords * 4u);
}

__device__ __forceinline__ void idle_wave(const WaveGeom& g) {
    for (uint32_t b = g.fast_begin; b <= g.end; b++) lds_barrier();
}

// Raw blocks [b0, fast_end): one asm loop (loads 2 blocks ahead into registers the compiler never allocates,
// schedule, K+W -> LDS).  Then the 1-2 padded tail blocks and the spare block, in C++.
template <typename Ops>
__device__ __forceinline__ void helper_wave(const TvPieces& p, const Ops& ops, const Group& q, uint32_t lds_lane,
                                            uint32_t wave) {
    const uint32_t b0 = q.g.fast_begin, end = q.g.end, fast_end = q.g.fast_end;
    uint32_t b = b0;
    if (fast_end > b0) {
        const uint8_t* va = q.piece + (uint64_t)b0 * 64;
#if TV_STAMPS
        LoopStamp st;
        st.start();
#if TV_SHA1_STAMP >= 2
        ops.helper_loop(va, fast_end - b0, lds_lane, st.bar, st.vm, st.lg);
#else
        ops.helper_loop(va, fast_end - b0, lds_lane, st.bar);
#endif
        st.end(p, wave, fast_end - b0);
#else
        ops.helper_loop(va, fast_end - b0, lds_lane);
#endif
        b = fast_end;
    }
    for (; b <= end; b++) {
        uint32_t w[16];
        build_tail_block(q.piece, q.len, b, w);
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = bswap32(w[i]);  // the schedule block byte-swaps
        ops.schedule_block(w, ring_buf(lds_lane, b - b0));
        if (b - b0 + 1 >= kAhead) lds_barrier();
    }
    for (uint32_t k = 1; k < kAhead; k++) lds_barrier();
}

// Blocks [b0, min(end, nb_min)), where every lane of the wave updates: one asm loop (rounds, h += r, barrier).  The
// rest only in a group with the short last piece: lanes past their final block keep their digest (both lanes of a
// twin pair hold the same piece and every lane runs every block's rounds, so the DPP partner is always in step).
template <typename Ops>
__device__ __forceinline__ void rounds_wave(const TvPieces& p, const Ops& ops, const Group& q, uint32_t lds_lane,
                                            uint32_t wave, uint32_t h[5]) {
    const uint32_t b0 = q.g.fast_begin, end = q.g.end;
    lds_barrier();
    uint32_t b = b0;
    const uint32_t full_end = end < q.g.nb_min ? end : q.g.nb_min;
    if (b < full_end) {
#if TV_STAMPS
        LoopStamp st;
        st.start();
        ops.rounds_loop(h, lds_lane, full_end - b, st.bar);
        st.end(p, wave, full_end - b);
#else
        ops.rounds_loop(h, lds_lane, full_end - b);
#endif
        b = full_end;
    }
    for (; b < end; b++) {
        uint32_t r[5];
        ops.rounds_block(h, r, ring_buf(lds_lane, b - b0));
        if (b < q.nb) {
#pragma unroll
            for (int i = 0; i < 5; i++) h[i] += r[i];
        }
        lds_barrier();
    }
}

}  // namespace

// A workgroup is PAIRS x {rounds, helper} waves over 64*PAIRS pieces.  Its waves go to distinct SIMDs, so with
// <= 1 workgroup per CU no rounds wave shares its SIMD.  Each pair has its own 3 x 20 KiB K+W ring; the barrier is
// workgroup-wide, so both pairs run the same (workgroup) block range.  LIST and BATCH: one pair per workgroup.
template <bool HASH, int PAIRS, int MODE = RESIDENT>
__global__ __launch_bounds__(128 * PAIRS) void tv_split_kernel(TvPieces p) {
    constexpr bool LISTED = MODE != RESIDENT;   // entries answered one byte each (finish_list), whole pieces only
    static_assert(!LISTED || PAIRS == 1, "list and batch mode run one pair per workgroup");
    __shared__ __attribute__((aligned(16))) uint4 ring[kBufs * PAIRS * kRingWords / 4];
    ClockStamp clk;
    clk.start(p);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t pair = wave % PAIRS;
    const uint32_t role = wave / PAIRS;        // 0 = rounds, 1 = helper
    const Group q = resolve_group<MODE>(p, blockIdx.x, 64u * PAIRS, pair * 64u + lane);
    const uint32_t lds_lane = (uint32_t)(uintptr_t)(void*)(ring + pair * kBufs * (kRingWords / 4)) + lane * 16u;
    const SplitOps ops;
    if (role != 0) {
        helper_wave(p, ops, q, lds_lane, wave);
        return;
    }
    uint32_t h[5];
    start_state<LISTED>(p, q.jj, h);
    rounds_wave(p, ops, q, lds_lane, wave, h);
    if (LISTED) finish_list(p, q.j < p.n, q.j, q.jj, h);
    else finish<HASH>(p, q.last_grp ? (lane == 0 && pair == 0) : q.j < p.n_main, q.jj, q.g0 + pair * 64u, h, q.last_grp);
    clk.end(p);   // (wave 0 is a rounds wave)
}

// ------------------------------------------------------------------------------------------
// twin kernel: the split kernel with TWO lanes per piece in every wave.  A workgroup is rounds waves 0, 1
// and helper waves 2, 3 over 64 pieces.  Helper: lane 2i + b runs piece 32(wave & 1) + i and owns its schedule
// words of parity b (tools/gen_sha1_asm.py gen_helper2).  Rounds: lanes 16r + k and 16r + 8 + k (k < 8) are
// roles 0 and 1 of piece 32(wave & 1) + 8r + k; of every two rounds role 0 computes the first and role 1 the
// second, from one F and one `F + e + KW` for both, and the rotl5-and-add chain passes between them through DPP
// (row_ror:8): 9 instructions per two rounds (gen_roles).  Role b reads only helper lane 2i + b's K+W words: 10
// ds_read_b128 per block instead of 20.  The loop over the full blocks runs two blocks per trip on two register
// sets for the K+W quads: serial stream 367 VALU + 10 LDS + 1 wait + barrier per block and one s_sub +
// s_cbranch per two blocks.  Every lane of a rounds wave stays active through all of its blocks (lanes past
// their piece's end run them too and discard the result).  Helper: 192 VALU + 10 ds_write_b128 per block
// (W[32..79] from the parity-closed recurrence W[t] = rotl2(W[t-6] ^ W[t-16] ^ W[t-28] ^ W[t-32])), half a
// split helper's stream.  K+W ring: 3 x 20 KiB, the helpers two blocks ahead, one workgroup barrier per block.
// Four waves per 64 pieces fill the SIMDs up to 16,384 pieces (cfg2: 256 workgroups, one per CU).
// ------------------------------------------------------------------------------------------
// Workgroup shapes (wave -> role and 32-piece half; the hardware puts a workgroup's waves on SIMDs in the
// cyclic order 0 -> 2 -> 1 -> 3 from a varying start, MI355X_MICROARCH.md section LDS):
//   1: 2 waves {rounds, helper} over 32 pieces, two workgroups per CU (the auto shape)
//   2: 4 waves, rounds {0, 1}, helpers {2, 3} over 64 pieces      3: rounds {0, 2}, helpers {1, 3}
//   4: 4 waves over 32 pieces, rounds 0, helper 2, waves 1 and 3 idle at the barriers   5: helper 1, idle 2, 3
// (shapes 3-5 are SIMD-placement probes: tools/twin_occupancy_probe.py)
constexpr int kTwinRole[6][4] = {{0, 0, 0, 0}, {0, 1, 2, 2}, {0, 0, 1, 1}, {0, 1, 0, 1}, {0, 2, 1, 2}, {0, 1, 2, 2}};
constexpr int kTwinHalf[6][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 1, 0, 1}, {0, 0, 1, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}};
constexpr int kTwinWaves[6] = {0, 2, 4, 4, 4, 4};
constexpr int kTwinPairs[6] = {0, 1, 2, 2, 1, 1};

template <bool HASH, int SHAPE, int MODE = RESIDENT>
__global__ __launch_bounds__(64 * kTwinWaves[SHAPE]) void tv_twin_kernel(TvPieces p) {
    constexpr bool LISTED = MODE != RESIDENT;   // (as in tv_split_kernel)
    __shared__ __attribute__((aligned(16))) uint4 ring[kBufs * kRingWords / 4];
    constexpr uint32_t span = 32u * kTwinPairs[SHAPE];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int role = kTwinRole[SHAPE][wave];                  // 0 rounds, 1 helper, 2 idle
    const uint32_t half = kTwinHalf[SHAPE][wave];             // pieces 32*half .. +31 of the group
    // companions (blockIdx past the real grid, TV_OPT_TWIN_FILL): re-hash main workgroup (blockIdx - real) % main
    const uint32_t nmain_wgs = ((LISTED ? p.n : p.n_main) + span - 1) / span;
    const uint32_t real_wgs = nmain_wgs + (!LISTED && p.n_main < p.n ? 1u : 0u);
    const bool companion = blockIdx.x >= real_wgs;
    const uint32_t wgi = companion ? (blockIdx.x - real_wgs) % nmain_wgs : blockIdx.x;
    // a companion keeps the instruction stream of the workgroup it copies but, unless fill_all, points every
    // lane at that workgroup's first piece: the same loads, one piece's bytes instead of 32 pieces'
    // the wave's piece of this lane, and the lane's half of it: helper lane 2i + b has parity b of piece i; rounds
    // lane 16r + 8b + k (k < 8) is role b of piece 8r + k, and reads what helper lane 2i + b wrote
    const uint32_t part = role == 0 ? (lane >> 3) & 1u : lane & 1u;
    const uint32_t pc = role == 0 ? (lane >> 4) * 8u + (lane & 7u) : lane >> 1;
    const Group q = resolve_group<MODE>(p, wgi, span, companion && !p.fill_all ? 0u : half * 32u + pc);
    const uint32_t lds_lane = (uint32_t)(uintptr_t)(void*)ring + half * 1024u + (2u * pc + part) * 16u;
    ClockStamp clk;
    clk.start(p);
    if (role == 2) {
        idle_wave(q.g);
        return;
    }
    const TwinOps ops{(lane & 1u) ? 0x07060504u : 0x03020100u};   // (read by helper lanes only)
    if (role == 1) {
        helper_wave(p, ops, q, lds_lane, wave);
        return;
    }
    uint32_t h[5];
    start_state<LISTED>(p, q.jj, h);
    rounds_wave(p, ops, q, lds_lane, wave, h);
    clk.end(p);              // (wave 0 is a rounds wave in every shape)
    if (companion) return;   // its digests duplicate a main workgroup's: nothing to write
    const bool role0 = part == 0;   // one writer per lane pair
    if (LISTED) finish_list(p, role0 && q.j < p.n, q.j, q.jj, h);
    else finish<HASH, true>(p, q.last_grp ? (wave == 0 && lane == 0) : (role0 && q.j < p.n_main), q.jj,
                            q.g0 + half * 32u, h, q.last_grp);
}

// ------------------------------------------------------------------------------------------
// list kernel (incremental verify): lane j verifies shard piece idx[j]; same compression path as
// the lane kernel.  MODE: LIST, or BATCH (launch position j is any torrent's piece, see resolve_group).
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void tv_list_kernel(TvPieces p) {
    const uint32_t gw = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (gw * 64u >= p.n) return;   // (the grid is whole 4-wave workgroups)
    const Group q = resolve_group<MODE>(p, gw, 64u, threadIdx.x & 63u);
    const WaveGeom& g = q.g;
    const uint8_t* piece = q.piece;
    uint32_t h[5];
    start_state<true>(p, q.jj, h);
    uint32_t b = 0, w[16];   // (a list launch covers whole pieces, see resolve_group: block 0, not blk_begin)
    if (b < g.fast_end) {
        const uint32_t last = g.fast_end - 1;
        uint4 A[4], B[4];
        load_block(piece, 0, A);
        load_block(piece, 1 < last ? 1 : last, B);
        for (;;) {
            bswap_block(A, w);
            load_block(piece, b + 2 < last ? b + 2 : last, A);
            compress_full(h, w);
            if (++b >= g.fast_end) break;
            bswap_block(B, w);
            load_block(piece, b + 2 < last ? b + 2 : last, B);
            compress_full(h, w);
            if (++b >= g.fast_end) break;
        }
    }
    for (; b < g.end; b++) {
        build_tail_block(piece, q.len, b, w);
        uint32_t r[5];
        tv_sha1_full(h, r, w, TV_K0, TV_K1, TV_K2, TV_K3);
        if (b < q.nb) {
#pragma unroll
            for (int i = 0; i < 5; i++) h[i] += r[i];
        }
    }
    finish_list(p, q.j < p.n, q.j, q.jj, h);
}

// ------------------------------------------------------------------------------------------
// synthetic payload fill: byte at linear offset o = byte (o & 7) of splitmix64(seed, o >> 3).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// L % 8 == 0: whole 8-byte words.  Piece j of the launch = global piece first + j.
__global__ __launch_bounds__(256) void tv_fill_words_kernel(uint8_t* payload, uint64_t stride, uint64_t first,
                                                            uint32_t n, uint64_t L, uint64_t seed) {
    const uint64_t wpp = L / 8;
    const uint64_t total = wpp * n;
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256ull) {
        const uint64_t j = g / wpp, k = g - j * wpp;
        const uint64_t o = (first + j) * L + 8 * k;
        *reinterpret_cast<uint64_t*>(payload + j * stride + 8 * k) = splitmix64(seed, o >> 3);
    }
}

__global__ __launch_bounds__(256) void tv_fill_bytes_kernel(uint8_t* payload, uint64_t stride, uint64_t first,
                                                            uint32_t n, uint64_t L, uint64_t seed) {
    const uint64_t total = L * n;
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256ull) {
        const uint64_t j = g / L, k = g - j * L;
        const uint64_t o = (first + j) * L + k;
        payload[j * stride + k] = (uint8_t)(splitmix64(seed, o >> 3) >> (8 * (o & 7)));
    }
}

// ------------------------------------------------------------------------------------------
// windowed layouts (tv_core.hip): the windows are hashed (HASH kernels into the shard's digest rows) as they
// fill, and tv_verify compares the whole shard at the end -- 40 B read per piece, one word written per 64.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tv_compare_kernel(const uint32_t* hash, const uint32_t* digests,
                                                         uint32_t dcount, uint32_t n, const uint64_t* avail64,
                                                         uint64_t* out64) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    bool ok = j < n;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 5; k++) ok &= hash[(uint64_t)k * dcount + j] == digests[(uint64_t)k * dcount + j];
    }
    const uint64_t mask = __ballot(ok);
    if ((threadIdx.x & 63u) == 0) {   // lane 0 of the wave: pieces j .. j + 63, word j >> 6
        uint64_t bits = __builtin_bswap64(__builtin_bitreverse64(mask));   // ballot bit l -> MSB-first bytes
        if (avail64) bits &= avail64[j >> 6];
        out64[j >> 6] = bits;
    }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called by tv_core.hip, tv_stream.hip, tv_verify.hip)
// ------------------------------------------------------------------------------------------
namespace {

// Calls f(std::bool_constant<hash>, std::integral_constant<int, v>) for the one v of Vs... that equals `v`, so
// that a launcher names a kernel template once and gets its HASH x variant instantiations.
template <int... Vs, typename F>
void dispatch(bool hash, int v, F f) {
    auto one = [&](auto V) {
        if (v != V()) return;
        if (hash) f(std::true_type{}, V);
        else f(std::false_type{}, V);
    };
    (one(std::integral_constant<int, Vs>{}), ...);
}

template <typename K>
void launch(K kernel, unsigned grid, unsigned block, hipStream_t s, const TvPieces& p) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, p);
}

}  // namespace

hipError_t tv_launch_verify(const TvPieces& p, int kernel, bool hash, hipStream_t s, int split_pairs,
                            uint32_t* workgroups) {
    if (workgroups) *workgroups = 0;
    if (p.n == 0) return hipSuccess;
    unsigned grid;
    if (kernel == TV_KERNEL_SPLIT) {
        // one pair per workgroup: with its 60 KiB LDS ring at most two workgroups share a CU, and up to
        // 32,768 pieces every rounds wave still gets a SIMD of its own; 1 pair beats 2 pairs (one 4-wave
        // barrier couples more jitter) at every piece count up to there, by 1.7-3 % (profiles/r02/sweep_3buf.log)
        const int pairs = split_pairs == 2 ? 2 : 1;
        grid = (p.n_main + 64 * pairs - 1) / (64 * pairs) + (p.n_main < p.n ? 1 : 0);
        dispatch<1, 2>(hash, pairs, [&](auto H, auto V) {
            launch(tv_split_kernel<H(), V()>, grid, 128 * V(), s, p);
        });
    } else if (kernel == TV_KERNEL_TWIN) {
        // split_pairs: (rounds, helper) pairs per workgroup: 1 (auto) = 2-wave workgroups over 32 pieces, two
        // per CU; 2 = the 4-wave workgroup over 64 pieces, whose 4-wave barrier couples more jitter (cfg2
        // 1,419 vs 1,358 GB/s, profiles/r02/sweep_twin.log)
        // (3-5: SIMD-placement probe shapes, see tv_twin_kernel)
        const int shape = split_pairs >= 2 && split_pairs <= 5 ? split_pairs : 1;
        const unsigned span = 32u * kTwinPairs[shape];
        const unsigned real = (p.n_main + span - 1) / span + (p.n_main < p.n ? 1 : 0);
        grid = (p.fill_to > real && p.n_main > 0) ? p.fill_to : real;
        dispatch<1, 2, 3, 4, 5>(hash, shape, [&](auto H, auto V) {
            launch(tv_twin_kernel<H(), V()>, grid, 64 * kTwinWaves[V()], s, p);
        });
    } else {
        const unsigned waves = (p.n_main + 63) / 64 + (p.n_main < p.n ? 1 : 0);
        grid = (waves + 3) / 4;
        dispatch<0, 1>(hash, p.lane_pairs ? 1 : 0, [&](auto H, auto V) {
            launch(tv_lane_kernel<H(), V() != 0>, grid, 256, s, p);
        });
    }
    if (workgroups) *workgroups = grid;
    return hipGetLastError();
}

hipError_t tv_launch_verify_list(const TvPieces& p, int kernel, hipStream_t s, uint32_t* workgroups) {
    if (workgroups) *workgroups = 0;
    if (p.n == 0) return hipSuccess;
    unsigned grid;
    if (kernel == TV_KERNEL_TWIN) {
        const unsigned real = (p.n + 31) / 32;
        grid = p.fill_to > real ? p.fill_to : real;
        launch(tv_twin_kernel<false, 1, LIST>, grid, 128, s, p);
    } else if (kernel == TV_KERNEL_SPLIT) {
        grid = (p.n + 63) / 64;
        launch(tv_split_kernel<false, 1, LIST>, grid, 128, s, p);
    } else {
        grid = (p.n + 255) / 256;
        launch(tv_list_kernel<LIST>, grid, 256, s, p);
    }
    if (workgroups) *workgroups = grid;
    return hipGetLastError();
}

// One workgroup per group of tv_batch_span(kernel) positions (lane: four groups, one per wave); no companions.
hipError_t tv_launch_verify_batch(const TvPieces& p, int kernel, hipStream_t s, uint32_t* workgroups) {
    if (workgroups) *workgroups = 0;
    if (p.n == 0) return hipSuccess;
    unsigned grid;
    if (kernel == TV_KERNEL_TWIN) {
        grid = (p.n + 31) / 32;
        launch(tv_twin_kernel<false, 1, BATCH>, grid, 128, s, p);
    } else if (kernel == TV_KERNEL_SPLIT) {
        grid = (p.n + 63) / 64;
        launch(tv_split_kernel<false, 1, BATCH>, grid, 128, s, p);
    } else {
        grid = (p.n + 255) / 256;
        launch(tv_list_kernel<BATCH>, grid, 256, s, p);
    }
    if (workgroups) *workgroups = grid;
    return hipGetLastError();
}

hipError_t tv_launch_fill(uint8_t* payload, uint64_t stride, uint64_t first, uint32_t n, uint64_t L,
                          uint64_t seed, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned grid = 256 * 32;
    if (L % 8 == 0) hipLaunchKernelGGL(tv_fill_words_kernel, dim3(grid), dim3(256), 0, s, payload, stride, first, n, L, seed);
    else hipLaunchKernelGGL(tv_fill_bytes_kernel, dim3(grid), dim3(256), 0, s, payload, stride, first, n, L, seed);
    return hipGetLastError();
}

hipError_t tv_launch_compare(const uint32_t* hash, const uint32_t* digests, uint32_t dcount, uint32_t n,
                             const uint64_t* avail64, uint64_t* out64, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tv_compare_kernel, dim3((n + 255) / 256), dim3(256), 0, s, hash, digests, dcount, n, avail64, out64);
    return hipGetLastError();
}
