// tv_plan.h -- the resident payload's shape under a device budget (tv_set_layout), a stream's windows x columns under
// one (stream_geometry; v2_stream_geometry for a BitTorrent v2 stream), the file table's walk (walk_file_table) and a
// v2 torrent's aligned file offsets (v2_file_starts) and the item list of a v2 block launch (v2_block_items,
// v2_block_scatter), the digest-word codec (digest_pack, digest_unpack), the launch order of a v1 list (list_plan)
// and the tail table of a hybrid call (hybrid_tails) and a hybrid stream's geometry and column pad ranges
// (hybrid_stream_geometry, hybrid_col_range), the pad chunks of a hybrid list entry (hybrid_list_chunk;
// tests/c/plan_hybrid_list_main.cpp, tests/test_plan_hybrid_list.py) and the stream engine's copy plan and row walk
// (for_row_copies, walk_row_files) and the launch order and group geometry of a batch (batch_plan;
// tests/c/plan_batch_main.cpp, tests/test_plan_batch.py), as plain host code with no HIP in it, so they are unit-tested
// on the CPU (tests/c/plan_test.cpp, tests/c/walk_main.cpp, tests/c/plan_v2_main.cpp, tests/c/plan_v2_blocks_main.cpp,
// tests/c/plan_codec_main.cpp, tests/c/plan_list_main.cpp, tests/c/plan_hybrid_main.cpp,
// tests/c/plan_hybrid_stream_main.cpp, tests/c/plan_stream_rows_main.cpp; tests/test_plan.py, test_plan_v2.py,
// test_plan_v2_blocks.py, test_plan_codec.py, test_plan_list.py, test_plan_hybrid.py, test_plan_hybrid_stream.py,
// test_plan_stream_rows.py).
// Also the file calls' path table (parse_path_table) and the short segments' slot packing and copy runs (pack_slot,
// for_copy_runs): tests/c/fileio_main.cpp, tests/test_fileio.py.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace tvi {

struct PayloadPlan {
    uint64_t bytes = 0;      // the allocation (0: none)
    bool win = false;        // windowed: `bufs` buffers of `win_n` pieces, `buf_bytes` each
    uint64_t win_n = 0;
    int bufs = 0;
    uint64_t buf_bytes = 0;
};

// Window buffers of a windowed layout by default (TV_OPT_WIN_BUFS = 0): window w + 1 stages while the two windows
// before it hash side by side, on the compute stream and one hash stream (a window's hash takes one piece's serial
// SHA-1 whatever its piece count, so under a small budget windows must hash side by side to keep staging busy).
// Three beat two and four at HIP's default 4 hardware queues: 0.5 GiB 28.3 / 22.2 / 26.5 GB/s, 1 GiB 51.6 / 38.5 /
// 45.2 (profiles/r06/window_bench_shipped_form.jsonl).
constexpr int kWinBufsDefault = 3;
constexpr int kWinBufsMax = 8;

// `count` pieces at `stride` bytes (+ `slack` after the last) under `budget` bytes: the whole shard when it fits,
// else `bufs` window buffers of W pieces (fewer buffers when the budget cannot hold one piece in each; never more
// than there are windows; W >= 1 even when one piece exceeds the budget; a multiple of 64 from 256 up, so each
// window is whole 64-piece waves).
inline PayloadPlan plan_payload(uint64_t count, uint64_t stride, uint64_t slack, uint64_t budget,
                                int bufs = kWinBufsDefault) {
    PayloadPlan p;
    if (count == 0) return p;
    p.bytes = count * stride + slack;
    if (p.bytes <= budget) return p;
    uint64_t B = (uint64_t)std::max(1, std::min(bufs, kWinBufsMax)), W = 0;
    for (; B > 1; B--) {
        W = budget / B > slack ? (budget / B - slack) / stride : 0;
        if (W) break;
    }
    if (B == 1) W = budget > slack ? (budget - slack) / stride : 0;
    W = std::max<uint64_t>(1, std::min(W, count));
    if (W >= 256) W = W / 64 * 64;
    B = std::max<uint64_t>(1, std::min(B, (count + W - 1) / W));
    p.win = true;
    p.win_n = W;
    p.bufs = (int)B;
    p.buf_bytes = W * stride + slack;
    p.bytes = B * p.buf_bytes;
    return p;
}

// Plan and allocate: try_alloc(plan, budget) -> 0 (the plan's bytes are held), 1 (out of memory), 2 (another
// failure).  Out of memory is retried with windows at half the budget while the request still shrinks and is
// above 64 MiB; a plan that cannot get smaller (a one-piece window of a piece larger than the memory left) is out of
// memory, not a retry forever.  Returns 0 (*out, *budget_out: what is held), 1 or 2; *failed_bytes:
// the last request that failed.
template <class TryAlloc>
int allocate_payload(uint64_t count, uint64_t stride, uint64_t slack, uint64_t budget, TryAlloc&& try_alloc,
                     PayloadPlan* out, uint64_t* budget_out, uint64_t* failed_bytes, int bufs = kWinBufsDefault) {
    uint64_t failed = UINT64_MAX;
    for (;;) {
        const PayloadPlan p = plan_payload(count, stride, slack, budget, bufs);
        const int r = try_alloc(p, budget);
        if (r == 0) {
            *out = p;
            *budget_out = budget;
            return 0;
        }
        *failed_bytes = p.bytes;
        if (r != 1 || p.bytes <= (64ull << 20) || p.bytes >= failed) return r;
        failed = p.bytes;
        budget = p.bytes / 2;  // windows of half the size
    }
}

// One segment of Storage.get's walk over a torrent's file table: `len` bytes of file `file` from byte `file_offset`
// are LINEAR bytes [linear, linear + len); len == 0 for the walk's zero-length segments.
struct TableSeg {
    uint64_t file, file_offset, linear, len;
};

// findAndDo's walk (storage.ts:98-137) over the files in order -- file k holds lengths[k] bytes and starts where the
// files before it end -- restricted to the LINEAR bytes [lo, hi) of a shard (lo a multiple of L): every segment with
// bytes there, and the zero-length segments fsStorage.get still opens (storage.ts:109-110,158): a file ending inside
// [lo, hi) that is empty or ends exactly where a piece starts.  The hosts' walks make the same list
// (torrent_amd/verify.py _files_shard over storage.py segment_arrays / zero_length_segments).  *reached: where the
// walk stopped (< hi: the files end before the shard does, and Storage.get returns null for a piece past their end).
// false (*bad = the file) when the lengths overflow 64-bit offsets.  tv_stage_file_table uses it;
// tests/c/walk_main.cpp runs it on the CPU.
inline bool walk_file_table(uint64_t n, const uint64_t* lengths, uint64_t lo, uint64_t hi, uint64_t L,
                            std::vector<TableSeg>* out, uint64_t* bad, uint64_t* reached) {
    uint64_t start = 0;
    for (uint64_t k = 0; k < n && start < hi; k++) {
        if (lengths[k] > UINT64_MAX - start) {
            *bad = k;
            return false;
        }
        const uint64_t end = start + lengths[k];
        const uint64_t a = std::max(lo, start), b = std::min(hi, end);
        if (b > a) out->push_back({k, a - start, a, b - a});
        if (end >= lo && end < hi && (lengths[k] == 0 || end % L == 0)) out->push_back({k, lengths[k], end, 0});
        start = end;
    }
    *reached = start;
    return true;
}

// The path table of the file-table calls: file k's path is the k-th NUL-terminated string of paths[0, paths_bytes)
// (bytes after the n-th string are ignored).  -> n with out[0..n) set, or the count of whole strings found (< n).
inline uint64_t parse_path_table(uint64_t n, const char* paths, uint64_t paths_bytes, const char** out) {
    uint64_t o = 0;
    for (uint64_t k = 0; k < n; k++) {
        const void* z = o < paths_bytes ? memchr(paths + o, 0, paths_bytes - o) : nullptr;
        if (!z) return k;
        out[k] = paths + o;
        o = (uint64_t)((const char*)z - paths) + 1;
    }
    return n;
}

// A short file segment of tv_stage_files (segment k of the call): file bytes [file_offset, file_offset + len) are
// LINEAR bytes [linear, linear + len), read into a ring slot at byte `packed`.
struct SmallSeg {
    uint64_t k, file_offset, linear, len, packed;
};

// Pack segments s[i..] into one slot of slot_bytes: each at the next byte whose offset agrees with its linear offset
// mod 4 (a dword-aligned DMA), while they fit.  -> j: s[i, j) are packed (their `packed` set).
inline size_t pack_slot(std::vector<SmallSeg>& s, size_t i, uint64_t slot_bytes) {
    uint64_t used = 0;
    size_t j = i;
    for (; j < s.size(); j++) {
        const uint64_t at = used + ((s[j].linear - used) & 3);
        if (at + s[j].len > slot_bytes) break;
        s[j].packed = at;
        used = at + s[j].len;
    }
    return j;
}

// One copy per run of readable (ok(q)), linear-contiguous segments of s[i, j) (packed by pack_slot: contiguous in the
// slot too): copy(q, r) for the run s[q, r); a nonzero return ends the walk and is returned.
template <class Ok, class Copy>
int for_copy_runs(const std::vector<SmallSeg>& s, size_t i, size_t j, Ok&& ok, Copy&& copy) {
    for (size_t q = i; q < j;) {
        if (!ok(q)) { q++; continue; }
        size_t r = q + 1;
        while (r < j && ok(r) && s[r].linear == s[r - 1].linear + s[r - 1].len) r++;
        if (const int rc = copy(q, r)) return rc;
        q = r;
    }
    return 0;
}

// ---- a stream request's copies and a row's files (tv_stream.hip: stream_commit_locked, stream_files_locked) ---------
//
// The copy plan of a request of n rows of `width` bytes, row q holding bytes(q) <= width valid ones: emit(first_row,
// rows, bytes_per_row) once per maximal run of full-width rows (one 2D copy), once per short row (a copy of its own),
// never for an empty row; a nonzero return ends the walk and is returned.  (A v1 request: at most a run and a tail.)
template <class Bytes, class Emit>
int for_row_copies(uint64_t n, uint64_t width, Bytes&& bytes, Emit&& emit) {
    for (uint64_t q = 0; q < n;) {
        const uint64_t nb = bytes(q);
        uint64_t e = q + 1;
        if (nb == width)
            while (e < n && bytes(e) == width) e++;
        if (nb)
            if (const int rc = emit(q, e - q, nb)) return rc;
        q = e;
    }
    return 0;
}

// A row's LINEAR bytes [a, b) over the file table: file k holds [start[k], start[k] + lengths[k]), start ascending with
// n + 1 entries (v1: the files back to back; v2: v2_file_starts, a gap after a file that does not end a piece).
// seg(file, file_offset, dst_offset, len) for each file segment in order; false from it stops the walk (kRowShort).
// Starts at the last k with start[k] <= a, skips the files that end at or before the position (zero-length ones among
// them), stops with kRowGap where the position lies before file k (the table and the rows disagree) and quietly where
// the table ends before b (the callers dealt with those pieces beforehand).
enum RowWalk { kRowWalked = 0, kRowGap = 1, kRowShort = 2 };
template <class Seg>
RowWalk walk_row_files(const uint64_t* start, const uint64_t* lengths, uint64_t n, uint64_t a, uint64_t b, Seg&& seg) {
    const uint64_t at = (uint64_t)(std::upper_bound(start, start + n + 1, a) - start);
    uint64_t k = at ? at - 1 : 0;
    for (uint64_t pos = a; pos < b && k < n; k++) {
        if (start[k] + lengths[k] <= pos) continue;
        if (pos < start[k]) return kRowGap;
        const uint64_t e = std::min(b, start[k] + lengths[k]);
        if (!seg(k, pos - start[k], pos - a, e - pos)) return kRowShort;
        pos = e;
    }
    return kRowWalked;
}

// ---- a stream's geometry under a device budget (tv_stream.hip: tv_stream_file_table, tv_verify_host) ----------------
//
// Windows of at least `min_win` pieces (a multiple of 64 unless the shard is smaller), each hashed column by column --
// enough pieces that a column hashes faster than it stages (2,048 pieces x 64 B per ~0.75 us block step: ~175 GB/s)
// -- and columns as wide as two chunk buffers within the budget allow, so each row is one long read or DMA row: 124 KiB
// at a 0.5 GiB budget and 1 MiB pieces where columns across all 16,384 pieces would be 16 KiB.  A multiple of 4 KiB
// from 4 KiB up (a cold file's rows are read O_DIRECT straight into the ring slot); where whole pieces fit, the
// windows grow to fill the budget.  Each chunk buffer is at most kStreamChunkMax: wider columns gained nothing and
// larger units overlap less (the first unit's copy and the last unit's kernel run alone): budgets of 2 GiB (1 GiB
// units) ran 44-49 GB/s against 52-55 at 0.5 GiB (profiles/r06/window_bench_payload_cols*.jsonl).  `slot` bounds a
// row (one ring slot), `slack` is the bytes after the last row.
constexpr uint64_t kStreamChunkMax = 256ull << 20;
inline void stream_geometry(uint64_t L, uint64_t count, uint64_t budget, uint64_t min_win, uint64_t slot,
                            uint64_t slack, uint64_t* col, uint64_t* win) {
    const uint64_t half = std::min<uint64_t>(budget / 2, kStreamChunkMax);
    const uint64_t lpad = std::min<uint64_t>((L + 63) / 64 * 64, slot);
    uint64_t w = std::min<uint64_t>(count, min_win);
    const uint64_t per = half > slack && w ? (half - slack) / w : 0;
    const uint64_t wid = per > 256 ? per - 256 : 64;
    uint64_t C = std::max<uint64_t>(64, std::min<uint64_t>(wid >= 4096 ? wid / 4096 * 4096 : wid / 64 * 64, lpad));
    if (C == lpad && w < count && half > slack)
        w = std::min<uint64_t>(count, std::max<uint64_t>(w, (half - slack) / (C + 256) / 64 * 64));
    *col = C;
    *win = w;
}

// ---- a BitTorrent v2 stream's geometry (tv_stream.hip: tv_v2_stream_begin, tv_v2_stream_file_table) ----------------
//
// A column is C bytes of every piece of a window of wn pieces: C a power of two, 16 KiB (one leaf) <= C <= Cmax =
// min(L, 64 MiB: one ring slot), so a column of a piece is a whole aligned subtree of c = C / 16 KiB leaves, which one
// workgroup reduces to one node; wn a multiple of 64 (bitfield words of its own), or the whole shard.
//   chunk > 0 (TV_OPT_STREAM_CHUNK): C = the largest power of two <= min(max(chunk, 16 KiB), Cmax), one window across
//     the shard.
//   chunk == 0: under `budget` bytes for the two chunk buffers (rows of pitch C + 256, `slack` after the last): start
//     from C = Cmax (whole pieces: the longest rows, no partial nodes), halve C while 64 rows do not fit, then wn = the
//     largest multiple of 64, at least 64 and at most the shard, whose two buffers fit.
// The serial unit of a v2 piece is a 16 KiB leaf, so a narrow window costs no serial hashing time: there is no floor
// of 2,048 pieces as in stream_geometry.  L must be a power of two >= 16 KiB (the callers check).
constexpr uint64_t kV2Leaf = 16384;
constexpr uint64_t kV2StreamColMax = 64ull << 20;
inline void v2_stream_geometry(uint64_t L, uint64_t count, uint64_t budget, uint64_t chunk, uint64_t slack,
                               uint64_t* col, uint64_t* win) {
    const uint64_t cmax = std::min<uint64_t>(L, kV2StreamColMax);
    if (chunk) {
        const uint64_t lim = std::min<uint64_t>(std::max<uint64_t>(chunk, kV2Leaf), cmax);
        uint64_t C = kV2Leaf;
        while (C * 2 <= lim) C *= 2;
        *col = C;
        *win = count;
        return;
    }
    const uint64_t half = budget / 2;
    auto fits = [&](uint64_t C, uint64_t rows) { return half >= slack && rows <= (half - slack) / (C + 256); };
    uint64_t C = cmax;
    while (C > kV2Leaf && !fits(C, 64)) C /= 2;
    uint64_t wn = half > slack ? (half - slack) / (C + 256) / 64 * 64 : 0;
    wn = std::max<uint64_t>(64, wn);
    *col = C;
    *win = std::min<uint64_t>(wn, count);
}

// Where each file of a v2 torrent starts in the ALIGNED linear space: every file starts a new piece, so
// start[k + 1] = round_up(start[k] + lengths[k], L) (a zero-length file takes no space).  start gets n + 1 entries;
// start[n] / L is the files' piece count.  false (*bad = the file) when the offsets overflow 64 bits.
inline bool v2_file_starts(uint64_t n, const uint64_t* lengths, uint64_t L, std::vector<uint64_t>* start,
                           uint64_t* bad) {
    start->assign(n + 1, 0);
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t s = (*start)[k];
        if (lengths[k] > UINT64_MAX - s || s + lengths[k] > UINT64_MAX - (L - 1)) {
            *bad = k;
            return false;
        }
        (*start)[k + 1] = (s + lengths[k] + L - 1) / L * L;
    }
    return true;
}

// ---- a v2 stream's device table (tv_stream.hip: v2_stream_begin_locked, v2_top_launch, stream_hash_end_locked) --------
//
// One table of 11 words per shard piece: three rows of `count` words (piece bytes, tree leaves, top-tree widths), then
// eight hash words per piece, SoA [8][wcount] window after window, so a window's finish launch sees a table of its own
// (pitch wcount) at the window's base.  A verify stream holds the expected roots there (the host packs them), a
// creation stream the roots its finish launches write (tv_stream_hash_end reads them back): the same words, so a
// creation stream needs no further buffer.  Windows are wn pieces, the last one the rest.
inline uint64_t v2s_tab_words(uint64_t count) { return 11 * count; }
// the words of the hash region: eight per shard piece
inline uint64_t v2s_hash_words(uint64_t count) { return 8 * count; }
// the word of the table at which the hash rows of the window starting at shard piece j0 begin (j0 a multiple of wn)
inline uint64_t v2s_hash_base(uint64_t count, uint64_t j0) { return 3 * count + 8 * j0; }
// hash word q (0 .. 7) of shard piece j in the hash region (index from v2s_hash_base(count, 0))
inline uint64_t v2s_hash_word(uint64_t count, uint64_t wn, uint64_t j, uint32_t q) {
    const uint64_t j0 = j / wn * wn, wcount = std::min(wn, count - j0);
    return 8 * j0 + (uint64_t)q * wcount + (j - j0);
}
// A window's top tree over the column nodes: level buffer A is [8][wcount x ncol] words, B follows it at this word
// ([8][wcount x max(ncol / 2, 1)]); both fit v2_node_words(wn, ncol) of any window of the stream.
inline uint64_t v2s_nodes_b_base(uint64_t wcount, uint64_t ncol) { return 8 * wcount * ncol; }

// ---- the item list of a v2 block launch (tv_v2.hip: tv_v2_leaf_hashes, tv_v2_check_blocks) --------------------------
//
// Entry k is a piece of piece_bytes[k] valid bytes in a torrent whose full piece holds W blocks of 16 KiB.  Its block
// i holds bytes when i * 16 KiB < piece_bytes[k]; the last such block may be short.  An item is one block the launch
// hashes: (entry, block, bytes).  want_bits (optional): n rows of ceil(W / 8) bytes, MSB-first, bit i of row k = block
// i of entry k is wanted; NULL = every block that holds bytes.  A wanted position that holds no byte gives no item.
// skip (optional): skip[k] != 0 = entry k gives no item (a piece with no slot, an unreadable piece).  Items come in
// entry order, blocks ascending, so the lanes of a wave read addresses 16 KiB apart.
struct V2BlockItem {
    uint32_t entry, leaf, len;
};

inline uint64_t v2_block_pitch(uint64_t W) { return (W + 7) / 8; }

// false: more than `cap` items (*items is then unspecified).
inline bool v2_block_items(uint64_t n, const uint32_t* piece_bytes, uint64_t W, const uint8_t* want_bits,
                           const uint8_t* skip, uint64_t cap, std::vector<V2BlockItem>* items) {
    items->clear();
    const uint64_t pitch = v2_block_pitch(W);
    for (uint64_t k = 0; k < n; k++) {
        if (skip && skip[k]) continue;
        const uint64_t bytes = piece_bytes[k];
        const uint64_t held = std::min<uint64_t>((bytes + kV2Leaf - 1) / kV2Leaf, W);   // blocks that hold bytes
        const uint8_t* row = want_bits ? want_bits + k * pitch : nullptr;
        for (uint64_t i = 0; i < held; i++) {
            if (row && !((row[i >> 3] >> (7 - (i & 7))) & 1)) continue;
            if (items->size() >= cap) return false;
            const uint64_t lo = i * kV2Leaf;
            items->push_back({(uint32_t)k, (uint32_t)i, (uint32_t)std::min<uint64_t>(kV2Leaf, bytes - lo)});
        }
    }
    return true;
}

// The launch's results back to per-entry bit rows: ballots[t >> 6] bit (t & 63) = item t matched.  ok_bits gets n
// rows of ceil(W / 8) bytes, MSB-first; a bit with no item, and every spare bit, is 0.
inline void v2_block_scatter(uint64_t n, uint64_t W, const std::vector<V2BlockItem>& items, const uint64_t* ballots,
                             uint8_t* ok_bits) {
    const uint64_t pitch = v2_block_pitch(W);
    std::fill(ok_bits, ok_bits + n * pitch, (uint8_t)0);
    for (uint64_t t = 0; t < items.size(); t++)
        if ((ballots[t >> 6] >> (t & 63)) & 1)
            ok_bits[items[t].entry * pitch + (items[t].leaf >> 3)] |= (uint8_t)(0x80u >> (items[t].leaf & 7));
}

// ---- digest words -------------------------------------------------------------------------------------------------------
//
// The library keeps every digest (SHA-1: 5 words, SHA-256: 8) as big-endian 32-bit VALUES, struct of arrays: word k
// of the digest in column `col` of a table of row length `pitch` is tab[k * pitch + col].  A table inside a larger
// one (the expected rows of a piece table, a stream window's rows) is passed as the pointer to its first word.
inline void digest_pack(const uint8_t* d, uint32_t words, uint32_t* tab, uint64_t pitch, uint64_t col) {
    for (uint32_t k = 0; k < words; k++, d += 4)
        tab[k * pitch + col] = ((uint32_t)d[0] << 24) | ((uint32_t)d[1] << 16) | ((uint32_t)d[2] << 8) | (uint32_t)d[3];
}

inline void digest_unpack(const uint32_t* tab, uint64_t pitch, uint64_t col, uint32_t words, uint8_t* d) {
    for (uint32_t k = 0; k < words; k++, d += 4) {
        const uint32_t v = tab[k * pitch + col];
        d[0] = (uint8_t)(v >> 24); d[1] = (uint8_t)(v >> 16); d[2] = (uint8_t)(v >> 8); d[3] = (uint8_t)v;
    }
}

// ---- the launch order of a v1 list (tv_verify.hip: tv_verify_list) ------------------------------------------------------
//
// pieces: the n listed shard-relative pieces in the caller's order.  held (optional): held[k] != 0 = entry k holds a
// slot of a slot pool (NULL: every entry); the others were never staged and are not launched.  short_last: the
// shard-relative index of the torrent's SHORT last piece (piece.ts:16-19), UINT64_MAX when the shard has none.  Listed
// together with full pieces it goes into waves of its own: launch = [the other entries..., copies of launch[0] up to a
// multiple of 64, the last-piece entries...], so no wave mixes the short piece's padding blocks with the others' raw
// blocks (the slow path); a list of last-piece entries only, or of none, is launched in the caller's order, unpadded.
// origin[t] = the entry launch position t answers (-1: padding).
inline void list_plan(uint64_t n, const uint32_t* pieces, const uint8_t* held, uint64_t short_last,
                      std::vector<uint32_t>* launch, std::vector<int64_t>* origin) {
    launch->clear();
    origin->clear();
    uint64_t launched = 0, nlast = 0;
    for (uint64_t k = 0; k < n; k++)
        if (!held || held[k]) {
            launched++;
            nlast += pieces[k] == short_last;
        }
    const bool separate = nlast && nlast < launched;
    launch->reserve(launched + 64);
    origin->reserve(launched + 64);
    for (int part = 0; part < (separate ? 2 : 1); part++) {
        for (uint64_t k = 0; k < n; k++)
            if ((!held || held[k]) && (!separate || (pieces[k] == short_last) == (part == 1))) {
                launch->push_back(pieces[k]);
                origin->push_back((int64_t)k);
            }
        if (separate && part == 0)
            while (launch->size() % 64) {
                launch->push_back((*launch)[0]);
                origin->push_back(-1);
            }
    }
}

// ---- the tail table of a hybrid call (tv_hybrid.hip: tv_hybrid_verify, tv_hybrid_hash) --------------------------------
//
// In a hybrid torrent (v1 + v2 descriptions of one payload, BEP 47 pad files after every file that does not end a
// piece) the v1 linear space is the aligned space of the layout: v1 piece i is the piece_bytes[i] file bytes of v2
// piece i followed by the pad file's zeros out to v1_len(i) = min(L, total - i * L).  A TAIL is a shard piece with
// piece_bytes < v1_len (at most one per file): payload row `row` (shard-relative piece) must hold zeros in the row's
// bytes [begin, end) before the SHA-1 kernels read it.  One tv_hybrid_pad_kernel launch zeroes every tail, a workgroup
// per CHUNK of kHybridChunk bytes: chunk k of an entry is the bytes of [begin, end) inside [a0 + k * kHybridChunk,
// a0 + (k + 1) * kHybridChunk), a0 = begin rounded down to 16, so every chunk but an entry's first starts 16-byte
// aligned in a row whose base is (rows are 64-byte aligned: stride = round_up(L, 64) + a multiple of 64).  chunk0 is
// the entry's first chunk in the launch (the entries' chunk counts summed before it); *chunks their total.
// piece_bytes: the SHARD's entries (count of them, piece first + j at [j]).  A short last piece (v1_len = its bytes)
// gives no entry; a trailing pad (total a multiple of L, the last file not) gives one out to L.
// false: *bad = the shard-relative piece whose piece_bytes exceed v1_len (the table does not describe this layout), or
// UINT64_MAX when L exceeds kHybridMaxL (offsets in a row are 32-bit).
struct HybridTail {
    uint32_t row, begin, end, chunk0;
};
constexpr uint64_t kHybridChunk = 64ull << 10;
constexpr uint64_t kHybridMaxL = 1ull << 31;

#if defined(__HIPCC__)
#define TV_PLAN_HD __host__ __device__
#else
#define TV_PLAN_HD
#endif
TV_PLAN_HD inline uint64_t hybrid_v1_len(uint64_t total, uint64_t L, uint64_t i) {
    if (i > UINT64_MAX / L || i * L >= total) return 0;
    return total - i * L < L ? total - i * L : L;
}

inline bool hybrid_tails(uint64_t total, uint64_t L, uint64_t first, uint64_t count, const uint32_t* piece_bytes,
                         std::vector<HybridTail>* out, uint64_t* chunks, uint64_t* bad) {
    out->clear();
    *chunks = 0;
    if (L == 0 || L > kHybridMaxL) {
        *bad = UINT64_MAX;
        return false;
    }
    for (uint64_t j = 0; j < count; j++) {
        const uint64_t v1 = hybrid_v1_len(total, L, first + j), b = piece_bytes[j];
        if (b > v1) {
            *bad = j;
            return false;
        }
        if (b == v1) continue;
        const uint64_t a0 = b & ~15ull;
        out->push_back({(uint32_t)j, (uint32_t)b, (uint32_t)v1, (uint32_t)*chunks});
        *chunks += (v1 - a0 + kHybridChunk - 1) / kHybridChunk;
    }
    return true;
}

// What workgroup g of the pad launch does, shared by the kernel (tv_hybrid.hip) and the CPU test that replays it
// (tests/c/plan_hybrid_main.cpp).  hybrid_chunk_entry: the entry whose chunks hold g (the last with chunk0 <= g; n > 0).
// hybrid_chunk_range: the row bytes [*b, *e) of chunk g of entry t; false = none.  hybrid_split: byte ADDRESSES
// [pb, pe) as byte stores [pb, *va), 16-byte vector stores [*va, *ve) (both 16-byte aligned) and byte stores [*ve, pe).
TV_PLAN_HD inline uint32_t hybrid_chunk_entry(const HybridTail* tails, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;   // tails[lo].chunk0 <= g, and hi == n or tails[hi].chunk0 > g
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tails[mid].chunk0 <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
TV_PLAN_HD inline bool hybrid_chunk_range(const HybridTail& t, uint32_t g, uint64_t* b, uint64_t* e) {
    if (t.begin >= t.end || t.chunk0 > g) return false;
    const uint64_t c0 = (uint64_t)(t.begin & ~15u) + (uint64_t)(g - t.chunk0) * kHybridChunk;
    *b = c0 > t.begin ? c0 : t.begin;
    *e = c0 + kHybridChunk < t.end ? c0 + kHybridChunk : t.end;
    return *b < *e;
}
TV_PLAN_HD inline void hybrid_split(uint64_t pb, uint64_t pe, uint64_t* va, uint64_t* ve) {
    const uint64_t a = (pb + 15) & ~15ull;
    *va = a < pe ? a : pe;
    *ve = *va + ((pe - *va) & ~15ull);
}

// ---- a hybrid stream (tv_stream.hip: tv_hybrid_stream_begin, tv_hybrid_stream_file_table) ---------------------------
//
// Both hash sets over the chunk buffers of ONE stream, so the geometry satisfies both sides.  The v2 side: C a power
// of two, 16 KiB <= C <= min(L, 64 MiB), wn a multiple of 64 or the whole shard (a column of a piece is an aligned
// subtree; C is a multiple of 64, so the SHA-1 column launches take it as it is).
//   chunk > 0 (TV_OPT_STREAM_CHUNK): v2_stream_geometry's rule, one window across the shard.
//   chunk == 0: v2_stream_geometry's whole pieces, as many as fit, are wrong here: SHA-1 is serial per piece, and a
//     window of a few hundred pieces hashes slower than it stages (stream_geometry above).  So each chunk buffer is at
//     most half = min(budget / 2, kStreamChunkMax) and a window has at least w0 = min(count, kHybridStreamWin) pieces:
//     start from C = min(L, 64 MiB), halve C while C > 16 KiB and w0 rows of pitch C + 256 (+ slack) do not fit half;
//     wn = the largest multiple of 64 whose rows fit half, at least 64, at most count.  (kHybridStreamWin is v1's
//     floor; tools/hybrid_bench.py --stream measures the combined launch set against the two separate streams.)
constexpr uint64_t kHybridStreamWin = 2048;
inline void hybrid_stream_geometry(uint64_t L, uint64_t count, uint64_t budget, uint64_t chunk, uint64_t slack,
                                   uint64_t* col, uint64_t* win) {
    if (chunk) {
        v2_stream_geometry(L, count, budget, chunk, slack, col, win);
        return;
    }
    const uint64_t half = std::min<uint64_t>(budget / 2, kStreamChunkMax);
    const uint64_t w0 = std::min<uint64_t>(count, kHybridStreamWin);
    auto fits = [&](uint64_t C, uint64_t rows) { return half >= slack && rows <= (half - slack) / (C + 256); };
    uint64_t C = std::min<uint64_t>(L, kV2StreamColMax);
    while (C > kV2Leaf && !fits(C, w0)) C /= 2;
    uint64_t wn = half > slack ? (half - slack) / (C + 256) / 64 * 64 : 0;
    wn = std::max<uint64_t>(64, wn);
    *col = C;
    *win = std::min<uint64_t>(wn, count);
}

// The bytes of a row of column [offset, offset + C) that must read as zeros, column-relative: the piece's pad range
// [piece_bytes, v1_len) (v1_len: hybrid_v1_len) cut to the column.  Empty when *b >= *e.
TV_PLAN_HD inline void hybrid_col_range(uint64_t piece_bytes, uint64_t v1_len, uint64_t offset, uint64_t C, uint64_t* b,
                                        uint64_t* e) {
    const uint64_t lo = piece_bytes > offset ? piece_bytes - offset : 0;
    const uint64_t hi = v1_len > offset ? v1_len - offset : 0;
    *b = lo < C ? lo : C;
    *e = hi < C ? hi : C;
}

// The column pad launch (tv_hybrid_col_pad_kernel) is rows x chunks workgroups: workgroup (row, k) stores chunk k of
// the row's range, cut exactly as a tail entry's chunks are (hybrid_chunk_range on {row, b, e, chunk0 = 0}).
// hybrid_col_chunks: the chunks of a range (0: empty).  hybrid_col_chunk: the column-relative bytes [*cb, *ce) of chunk
// k of a row with piece_bytes valid bytes in a torrent of `total` v1 bytes; false = none.  Shared by the kernel and the
// CPU test that replays it (tests/c/plan_hybrid_stream_main.cpp).
TV_PLAN_HD inline uint64_t hybrid_col_chunks(uint64_t b, uint64_t e) {
    return b < e ? (e - (b & ~15ull) + kHybridChunk - 1) / kHybridChunk : 0;
}
TV_PLAN_HD inline bool hybrid_col_chunk(uint64_t piece_bytes, uint64_t total, uint64_t L, uint64_t piece,
                                        uint64_t offset, uint64_t C, uint32_t k, uint64_t* cb, uint64_t* ce) {
    uint64_t b, e;
    hybrid_col_range(piece_bytes, hybrid_v1_len(total, L, piece), offset, C, &b, &e);
    if (b >= e) return false;
    const HybridTail t{0, (uint32_t)b, (uint32_t)e, 0};
    return hybrid_chunk_range(t, k, cb, ce);
}

// ---- the pad launch of a hybrid list (tv_hybrid.hip: tv_hybrid_verify_list) -------------------------------------------
//
// A listed entry is a whole piece in a payload row or a slot: the column [0, L) of its piece.  The list pad launch
// (tv_hybrid_list_pad_kernel) is entries x chunks workgroups: workgroup (e, k) stores chunk k of the entry's pad range
// [piece_bytes, v1_len), cut by the column rule above with offset = 0 and C = L.  hybrid_list_chunks: the chunks of
// an entry (0: no pad range; the host takes the largest as the grid's y).  Shared by the kernel and the CPU test that
// replays it (tests/c/plan_hybrid_list_main.cpp).
TV_PLAN_HD inline uint64_t hybrid_list_chunks(uint64_t piece_bytes, uint64_t total, uint64_t L, uint64_t piece) {
    uint64_t b, e;
    hybrid_col_range(piece_bytes, hybrid_v1_len(total, L, piece), 0, L, &b, &e);
    return hybrid_col_chunks(b, e);
}
TV_PLAN_HD inline bool hybrid_list_chunk(uint64_t piece_bytes, uint64_t total, uint64_t L, uint64_t piece, uint32_t k,
                                         uint64_t* b, uint64_t* e) {
    return hybrid_col_chunk(piece_bytes, total, L, piece, 0, L, k, b, e);
}

// ---- the launch order and group geometry of a batch (tv_batch.hip: tv_batch_verify) -----------------------------------
//
// lens: the length of every piece of the batch, in (torrent, piece) order; span: the entries of a group of the chosen
// kernel form (32 twin, 64 split and lane).  The entries are launched longest first (a stable sort by SHA-1 block
// count, so neighbouring pieces of a torrent stay neighbours and the longest serial chains start first) in groups of
// `span` consecutive launch positions.  A group's waves run ONE block range (the kernels' barrier protocol), given by
// its record: raw blocks [0, fast_end) for every member, blocks up to `end` on the padded-block path, every member
// updating its digest below nb_min.  The padded-block path is the slow one, so a group is CLOSED EARLY when the next
// entry would make nb_max - nfull_min exceed max(kBatchCutBlocks, nb_max / kBatchCutShare) -- at most 1 / kBatchCutShare
// of a group's blocks run there -- and is then padded to `span` with copies of its own last entry (origin -1).  Both
// constants are design parameters, not measurements.  The last group is not padded: the kernels point its spare lanes
// at the launch's last entry, one of its members.
// fast_end * 64 <= len for every member of a group: no raw-block load leaves any member's bytes (the kernels' memory
// safety; tests/c/plan_batch_main.cpp, tests/test_plan_batch.py check it as an invariant).
struct BatchGroup {
    uint32_t fast_end, end, nb_min;   // min len / 64, max blocks, min blocks over the group's members
};
constexpr uint64_t kBatchCutBlocks = 8;
constexpr uint64_t kBatchCutShare = 8;
inline uint64_t sha1_blocks(uint64_t len) { return (len + 8) / 64 + 1; }   // (a piece of length 0 still has one)

// launch[t]: the entry launch position t hashes; origin[t]: the entry it answers (-1: padding); groups[g]: positions
// [g * span, (g + 1) * span).
inline void batch_plan(uint64_t n, const uint64_t* lens, uint32_t span, std::vector<uint32_t>* launch,
                       std::vector<int64_t>* origin, std::vector<BatchGroup>* groups) {
    launch->clear();
    origin->clear();
    groups->clear();
    std::vector<uint32_t> order(n);
    for (uint64_t k = 0; k < n; k++) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return sha1_blocks(lens[a]) > sha1_blocks(lens[b]); });
    for (uint64_t i = 0; i < n;) {
        const uint64_t nb_max = sha1_blocks(lens[order[i]]), cut = std::max(kBatchCutBlocks, nb_max / kBatchCutShare);
        uint64_t nfull_min = lens[order[i]] / 64, nb_min = nb_max;
        uint32_t taken = 0;
        for (; taken < span && i < n; taken++, i++) {
            const uint64_t len = lens[order[i]];
            if (nb_max - std::min(nfull_min, len / 64) > cut) break;   // (never the group's first entry: 1 or 2 <= cut)
            nfull_min = std::min(nfull_min, len / 64);
            nb_min = std::min(nb_min, sha1_blocks(len));
            launch->push_back(order[i]);
            origin->push_back((int64_t)order[i]);
        }
        if (i < n)   // closed early (or full): every group but the last is whole
            for (; taken < span; taken++) {
                launch->push_back(launch->back());
                origin->push_back(-1);
            }
        groups->push_back({(uint32_t)nfull_min, (uint32_t)nb_max, (uint32_t)nb_min});
    }
}

}  // namespace tvi
